// renderer.hpp — host mirror of the reference's Renderer (src/render/renderer.rs) with
// the SDF raster moved to the GPU.
//
//   Renderer::{new,new_precise,new_dummy}   renderer.rs:25-43
//   Renderer::prepare_glyph                 renderer.rs:64-91
//   Renderer::render_glyph                  renderer.rs:103-149
//   RenderResult / into_pbf_glyph           src/render/result.rs:7-29,66-76
//   renderer_dummy                          src/render/renderer_dummy.rs:3-5
//
// The reference dispatches `match self.mode { Precise => renderer_precise(..), Dummy => .. }`
// (renderer.rs:140-143).  Here Precise IS the HIP back-end: there is no CPU raster in this
// library.  render_glyph keeps the per-glyph API; the throughput path is the batched form
// (prepare -> GlyphBatch -> render_batch) that FontManager::render_glyphs drives.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <map>
#include <set>
#include <memory>
#include <new>
#include <atomic>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../../include/vgsdf.h"
#include "../upload_layout.h"
#include "geometry.hpp"
#include "pbf.hpp"
#include "ring_builder.hpp"
#include "ttf_face.hpp"

namespace vg {

constexpr int32_t GLYPH_SIZE = 24; // src/render/mod.rs:52
constexpr int32_t BUFFER = 3;      // mod.rs:58

// RenderResult (result.rs:7-29) + what into_pbf_glyph needs, minus the pixels
struct GlyphJob {
	uint32_t id = 0;
	uint32_t advance = 0;
	bool has_raster = false; // false => PbfGlyph::empty(id, advance)
	int32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
	uint32_t width = 0, height = 0; // including 2*BUFFER
	uint32_t n_segments = 0;

	// result.rs:66-76, with the `glyph.y1 -= GLYPH_SIZE` of renderer.rs:146 applied
	PbfGlyphRef to_pbf(const uint8_t *bitmap) const
	{
		PbfGlyphRef g;
		g.id = id;
		g.advance = advance;
		if (has_raster) {
			g.bitmap = bitmap;
			g.bitmap_len = (size_t)width * height;
			g.width = width - 2 * BUFFER;
			g.height = height - 2 * BUFFER;
			g.left = x0 + BUFFER;
			g.top = (y1 - GLYPH_SIZE) - BUFFER;
		}
		return g;
	}
};

// Host SoA batch in exactly the layout vgsdf_batch wants (include/vgsdf.h).
struct GlyphBatch {
	std::vector<GlyphJob> jobs;       // ALL glyphs, rasterised or empty, in submission order
	std::vector<uint32_t> raster_job; // index into jobs for each rasterised glyph
	std::vector<uint32_t> seg_off{0};
	std::vector<double> sx, sy, ex, ey;
	std::vector<int32_t> x0, y0;
	std::vector<uint32_t> w, h;
	std::vector<uint64_t> out_off{0};

	void clear();
	size_t n_raster() const { return w.size(); }
	uint64_t out_bytes() const { return out_off.back(); }
	vgsdf_batch view() const;
	// appends another batch (jobs keep their relative order)
	void append(const GlyphBatch &o);
};

// Grow-only host array; page-locked (vgsdf_host_alloc) when HIP is available so the device
// layer can DMA it without a staging copy, plain malloc otherwise (dummy renderer on CPU).
template <class T> class HostBuffer {
public:
	explicit HostBuffer(bool want_pinned = false) : want_pinned_(want_pinned) {}
	HostBuffer(const HostBuffer &) = delete;
	HostBuffer &operator=(const HostBuffer &) = delete;
	~HostBuffer() { release(); }
	// contents are NOT preserved across a growth
	void ensure(size_t n)
	{
		if (n <= cap_)
			return;
		release();
		const size_t want = n + n / 4 + 64;
		if (want_pinned_) {
			p_ = static_cast<T *>(vgsdf_host_alloc(want * sizeof(T)));
			pinned_ = p_ != nullptr;
		}
		if (!p_) {
			p_ = static_cast<T *>(std::malloc(want * sizeof(T)));
			if (!p_)
				throw std::bad_alloc();
		}
		cap_ = want;
	}
	T *data() { return p_; }
	const T *data() const { return p_; }
	size_t capacity() const { return cap_; }
	T &operator[](size_t i) { return p_[i]; }
	const T &operator[](size_t i) const { return p_[i]; }

private:
	void release()
	{
		if (p_) {
			if (pinned_)
				vgsdf_host_free(p_);
			else
				std::free(p_);
		}
		p_ = nullptr;
		cap_ = 0;
		pinned_ = false;
	}
	T *p_ = nullptr;
	size_t cap_ = 0;
	bool want_pinned_, pinned_ = false;
};

// The batch as the device boundary wants it (include/vgsdf.h), in reusable buffers; the big
// arrays (segments, output pixels) are page-locked.
struct PackedBatch {
	HostBuffer<uint32_t> seg_off;
	HostBuffer<double> sx{true}, sy{true}, ex{true}, ey{true};
	HostBuffer<int32_t> x0, y0;
	HostBuffer<uint32_t> w, h;
	HostBuffer<uint64_t> out_off;
	HostBuffer<uint8_t> out{true};
	uint32_t n_raster = 0;
	uint64_t n_seg = 0, out_bytes = 0;

	void reserve(uint32_t rasters, uint64_t segs, uint64_t pixels);
	vgsdf_batch view() const;
};

// Outline commands of a set of glyphs for the DEVICE front-end (vgsdf_outlines): the host
// records what ttf-parser's OutlineBuilder receives; flattening, ring rules, scale/shift and
// bbox then run on the GPU (csrc/outline_kernels.hip).
struct OutlineBatch {
	std::vector<GlyphJob> jobs;        // one per glyph the reference returns Some(..) for
	std::vector<uint32_t> cmd_off{0};  // [jobs + 1]
	std::vector<uint32_t> dat_off{0};  // [jobs + 1]: coordinates the commands carry (2 / 4 / 6 / 0 per move or line / quad / curve / close)
	std::vector<vgsdf_outline_cmd> cmds;
	std::vector<double> scale, shift_x;

	void clear()
	{
		jobs.clear();
		cmd_off.assign(1, 0);
		dat_off.assign(1, 0);
		cmds.clear();
		scale.clear();
		shift_x.clear();
	}
	vgsdf_outlines view() const
	{
		vgsdf_outlines o;
		o.n_glyphs = (uint32_t)jobs.size();
		o.cmd_off = cmd_off.data();
		o.cmds = cmds.data();
		o.scale = scale.data();
		o.shift_x = shift_x.data();
		return o;
	}
};

// The same, recorded straight in the compact upload form of vgsdf_outlines_packed (one kind byte per command plus only
// the coordinates its kind carries: ~12 bytes per command of a TrueType font instead of a 28-byte record): what the
// workers of FontManager write, so that merging their batches is a copy.
struct PackedOutlineBatch {
	std::vector<GlyphJob> jobs;
	std::vector<uint32_t> cmd_off{0}, dat_off{0}; // [jobs + 1] into kinds / coords
	std::vector<uint8_t> kinds;
	std::vector<float> coords;
	std::vector<double> scale, shift_x;
	void clear()
	{
		jobs.clear();
		cmd_off.assign(1, 0);
		dat_off.assign(1, 0);
		kinds.clear();
		coords.clear();
		scale.clear();
		shift_x.clear();
	}
};

// wait_outlines on a batch submitted in the glyf form: one of its `glyf` entries is malformed (VGSDF_E_GLYF) — the batch
// has to be recorded on the host, where ttf-parser's rules for such glyphs are applied
struct GlyfEntryError : std::runtime_error {
	using std::runtime_error::runtime_error;
};

// What a worker records for the device's glyf decoder (vgsdf_outlines_glyf): per glyph its metrics and the parts — the
// simple glyphs it is drawn from, their `glyf` arrays copied as they stand.  Offsets are relative to this batch.
struct GlyfPartsBatch {
	std::vector<GlyphJob> jobs;
	std::vector<uint32_t> slot_off{0}, part_off{0}; // [jobs + 1] command slots / parts
	std::vector<GlyfPart> parts;
	std::vector<uint8_t> bytes;
	std::vector<double> scale, shift_x;
	uint32_t slots = 0;
	bool overflow = false; // a glyph's parts passed what 32-bit offsets address (Face::glyph_parts): not a batch for the device
	void clear()
	{
		overflow = false;
		jobs.clear();
		slot_off.assign(1, 0);
		part_off.assign(1, 0);
		parts.clear();
		bytes.clear();
		scale.clear();
		shift_x.clear();
		slots = 0;
	}
};

// What is recorded for a submission that names its glyphs (vgsdf_outlines_resident): per glyph its metrics, the file of the
// font id that draws it and its glyph id there — no outline is walked, no font byte copied.
struct ResidentBatch {
	std::vector<GlyphJob> jobs;
	std::vector<uint16_t> font_of, glyph_id;
	std::vector<double> scale, shift_x;
	void clear()
	{
		jobs.clear();
		font_of.clear();
		glyph_id.clear();
		scale.clear();
		shift_x.clear();
	}
};

// The merged batch handed to the device, in the compact upload form (vgsdf_outlines_packed: one kind byte per
// command plus the coordinates its kind carries).  All arrays live back to back in ONE page-locked block, in the
// order vgsdf.h names for a single-copy upload: scale | shift_x | cmd_off | dat_off | (pad to 8) | coords | kinds
// (the offsets: ../upload_layout.h, which the device layer recognises the block by).
struct MergedOutlines {
	// (which layout the blob has, and so which of view() / view_glyf() / view_resident() hands it to the device, is the caller's
	// to remember)
	std::vector<GlyphJob> jobs;
	HostBuffer<uint8_t> blob{true};
	uint32_t n_jobs = 0;
	double *scale = nullptr, *shift_x = nullptr;
	uint32_t *cmd_off = nullptr, *dat_off = nullptr;
	float *coords = nullptr;
	uint8_t *kinds = nullptr;
	uint32_t *pbf_pre = nullptr; // in-place PBF assembly (vgsdf.h): bytes reserved in front of a glyph's entry
	uint8_t *pbf_fix = nullptr;  // ... and the lengths of its id / advance fields; NULL when `with_pbf` was false
	// the glyf form (vgsdf_outlines_glyf) in the same block: scale | shift_x | cmd_off | (pad to 8) | parts | bytes [| pbf_pre | pbf_fix]
	vgsdf_glyf_part *parts = nullptr;
	uint8_t *glyf_bytes = nullptr;
	uint32_t n_parts = 0, n_glyf_bytes = 0;
	// the forms that name their glyphs (vgsdf_outlines_resident): the per-glyph arrays where ResidentBlockLayout has them
	// (command fonts: CommandBlockLayout, no part_off between cmd_off and the names)
	uint16_t *glyph_id = nullptr, *font_of = nullptr;
	std::vector<const vgsdf_font *> fonts; // the device copies of the group's faces

	void layout_resident(uint32_t jobs_n, bool with_pbf, bool command_fonts = false)
	{
		if (command_fonts)
			place_named(jobs_n, vgsdf::CommandBlockLayout(jobs_n, fonts.size(), with_pbf), with_pbf);
		else
			place_named(jobs_n, vgsdf::ResidentBlockLayout(jobs_n, fonts.size(), with_pbf), with_pbf);
	}
	vgsdf_outlines_resident view_resident() const
	{
		vgsdf_outlines_resident o;
		o.n_glyphs = n_jobs;
		o.n_fonts = (uint32_t)fonts.size();
		o.fonts = fonts.data();
		o.font_of = font_of;
		o.glyph_id = glyph_id;
		o.scale = scale;
		o.shift_x = shift_x;
		o.pbf_pre = pbf_pre;
		o.pbf_fix = pbf_fix;
		return o;
	}
	void layout_glyf(uint32_t jobs_n, uint32_t parts_n, uint32_t bytes_n, bool with_pbf)
	{
		n_parts = parts_n;
		n_glyf_bytes = bytes_n; // (a multiple of 4: every part's bytes are padded)
		const vgsdf::GlyfBlockLayout at(jobs_n, parts_n, bytes_n, with_pbf);
		uint8_t *b = place_shared(jobs_n, at, with_pbf);
		parts = reinterpret_cast<vgsdf_glyf_part *>(b + at.parts);
		glyf_bytes = b + at.glyf_bytes;
	}
	vgsdf_outlines_glyf view_glyf() const
	{
		vgsdf_outlines_glyf o;
		o.n_glyphs = n_jobs;
		o.n_parts = n_parts;
		o.n_bytes = n_glyf_bytes;
		o.cmd_off = cmd_off;
		o.parts = parts;
		o.bytes = glyf_bytes;
		o.scale = scale;
		o.shift_x = shift_x;
		o.pbf_pre = pbf_pre;
		o.pbf_fix = pbf_fix;
		return o;
	}
	void layout(uint32_t jobs_n, uint32_t n_cmds, uint32_t n_floats, bool with_pbf = false)
	{
		const vgsdf::PackedBlockLayout at(jobs_n, n_cmds, n_floats, with_pbf);
		uint8_t *b = place_shared(jobs_n, at, with_pbf);
		dat_off = reinterpret_cast<uint32_t *>(b + at.dat_off);
		coords = reinterpret_cast<float *>(b + at.coords);
		kinds = b + at.kinds;
	}
	vgsdf_outlines_packed view() const
	{
		vgsdf_outlines_packed o;
		o.n_glyphs = n_jobs;
		o.cmd_off = cmd_off;
		o.dat_off = dat_off;
		o.kinds = kinds;
		o.coords = coords;
		o.scale = scale;
		o.shift_x = shift_x;
		o.pbf_pre = pbf_pre;
		o.pbf_fix = pbf_fix;
		return o;
	}

private:
	// The arrays every layout has — pbf_pre, pbf_fix, scale, shift_x, cmd_off — placed in a blob of the layout's size; the
	// packed form's own arrays are cleared, and the caller adds those of its form.  Returns the blob
	template <class Layout> uint8_t *place_shared(uint32_t jobs_n, const Layout &at, bool with_pbf)
	{
		n_jobs = jobs_n;
		blob.ensure(at.bytes + 16);
		uint8_t *b = blob.data();
		pbf_pre = with_pbf ? reinterpret_cast<uint32_t *>(b + at.pbf_pre) : nullptr;
		pbf_fix = with_pbf ? b + at.pbf_fix : nullptr;
		scale = reinterpret_cast<double *>(b + at.scale);
		shift_x = reinterpret_cast<double *>(b + at.shift_x);
		cmd_off = reinterpret_cast<uint32_t *>(b + at.cmd_off);
		dat_off = nullptr;
		coords = nullptr;
		kinds = nullptr;
		return b;
	}
	template <class Layout> void place_named(uint32_t jobs_n, const Layout &at, bool with_pbf)
	{
		uint8_t *b = place_shared(jobs_n, at, with_pbf);
		cmd_off = nullptr; // (the library sums the offsets itself)
		glyph_id = reinterpret_cast<uint16_t *>(b + at.glyph_id);
		font_of = reinterpret_cast<uint16_t *>(b + at.font_of);
	}
};

// OutlineBuilder sink that records the callbacks verbatim.
class CommandRecorder final : public OutlineBuilder {
public:
	explicit CommandRecorder(std::vector<vgsdf_outline_cmd> &out) : out_(out) {}
	void move_to(float x, float y) override { n_floats_ += 2, push(0, 0, 0, 0, 0, x, y); }
	void line_to(float x, float y) override { n_floats_ += 2, push(1, 0, 0, 0, 0, x, y); }
	void quad_to(float x1, float y1, float x, float y) override { n_floats_ += 4, push(2, x1, y1, 0, 0, x, y); }
	void curve_to(float x1, float y1, float x2, float y2, float x, float y) override { n_floats_ += 6, push(3, x1, y1, x2, y2, x, y); }
	void close() override { push(4, 0, 0, 0, 0, 0, 0); }
	uint32_t n_floats() const { return n_floats_; } // coordinates the recorded commands carry

private:
	uint32_t n_floats_ = 0;
	void push(uint32_t kind, float x1, float y1, float x2, float y2, float x, float y)
	{
		vgsdf_outline_cmd c;
		c.x1 = x1;
		c.y1 = y1;
		c.x2 = x2;
		c.y2 = y2;
		c.x = x;
		c.y = y;
		c.kind = kind;
		out_.push_back(c);
	}
	std::vector<vgsdf_outline_cmd> &out_;
};

// Per-thread scratch so tessellation allocates nothing in steady state.
struct TessScratch {
	RingBuilder builder;
};

class Renderer {
public:
	enum class Mode { Hip, Dummy };

	// renderer.rs:25-31
	static std::shared_ptr<Renderer> create(bool dummy, int device = 0, std::string *err = nullptr);
	static std::shared_ptr<Renderer> new_precise(int device = 0, std::string *err = nullptr); // HIP back-end
	static std::shared_ptr<Renderer> new_dummy();
	// ONE process, N devices (the reference is one process too, manager.rs:81-125): a HIP renderer on
	// devices[0] plus one peer per further entry, each with its own device contexts and streams.  An entry may repeat a
	// device (N lanes rehearsed on one GPU).  FontManager::render_glyphs deals a font's glyph shards to the lanes, one host
	// thread each; every single-renderer call on the object goes to devices[0].
	static std::shared_ptr<Renderer> new_multi(const std::vector<int> &devices, std::string *err = nullptr);
	size_t n_devices() const { return 1 + peers_.size(); }
	const Renderer &device_lane(size_t i) const { return i == 0 ? *this : *peers_[i - 1]; }
	// run counters {blocks, glyphs, pixels}: credited to the lane that did the work, summed over the lanes by
	// vgsdf_reduce_counters (an RCCL all-reduce when the lanes sit on distinct devices).  Hip mode only.
	void add_counters(uint64_t blocks, uint64_t glyphs, uint64_t pixels) const;
	void reset_counters() const;
	void reduce_counters(uint64_t out[3]) const;
	// how the last reduce_counters took its sum (vgsdf_reduce_path): "rccl", "host: ...", "host: RCCL fallback: <reason>"
	std::string reduce_path() const;
	~Renderer();

	Mode mode() const { return mode_; }
	int device() const { return device_; }

	// Host half of render_glyph, renderer.rs:103-137: cmap lookup, outline, flatten, scale,
	// sub-pixel shift, bbox + buffer.  nullopt = the reference returns None (glyph skipped).
	// Rasterised glyphs get their segments appended to `batch`.
	static bool prepare(const Face &face, uint32_t index, TessScratch &scratch, GlyphBatch &batch);

	// Host half for the DEVICE front-end: cmap lookup, advance, scale / shift, and the raw
	// outline commands (renderer.rs:104-116,130); everything else happens on the GPU.
	static bool record(const Face &face, uint32_t index, OutlineBatch &batch);
	static bool record(const Face &face, uint32_t index, PackedOutlineBatch &batch); // the same into the compact form
	// ... and for the device's glyf decoder: nothing is decoded, the glyph's simple glyphs are appended as parts
	// (glyf fonts only: face.has_glyf_form())
	static bool record_parts(const Face &face, uint32_t index, GlyfPartsBatch &batch);
	// the same for a resident face: the glyph is named, not walked (file = the face's index among the font id's files)
	static bool record_resident(const Face &face, uint16_t file, uint32_t index, ResidentBatch &batch);
	// Device front-end + raster for a recorded batch: fills rects (one per job) and `out` with
	// the bitmaps of the glyphs that have a raster, packed in job order.  Hip mode only.
	void render_outlines(const vgsdf_outlines &batch, std::vector<vgsdf_rect> &rects, HostBuffer<uint8_t> &out,
	                     uint64_t &out_bytes, uint64_t &n_segments) const;
	// The same in two halves on one of two lanes (each lane = its own device context and stream): submit enqueues
	// upload, front-end and raster and returns; wait collects.  A caller that alternates the lanes keeps the GPU
	// busy while it records the next batch and encodes the previous one.  `batch` (its command array) and `out`
	// must stay untouched between the two calls; a lane is held from submit to wait.
	void submit_outlines(int lane, const vgsdf_outlines_packed &batch, HostBuffer<uint8_t> &out) const;
	void submit_outlines(int lane, const vgsdf_outlines_glyf &batch, HostBuffer<uint8_t> &out) const;
	// ... and for glyphs named by (font, glyph id) of resident fonts; *block_bytes: what the submission uploaded
	// (mixed: `batch.fonts` holds stores of both kinds — vgsdf_outlines_submit_resident_mixed)
	void submit_outlines(int lane, const vgsdf_outlines_resident &batch, HostBuffer<uint8_t> &out, uint64_t *block_bytes = nullptr,
	                     bool mixed = false) const;
	// Resident fonts: the device copy of a face (vgsdf_font), one per (device, face), created on first use through the
	// lane's context, shared by the two contexts of a lane and by the lanes of a multi-device renderer that share a device,
	// freed with the renderer.  nullptr: the face has no resident form, or its copy would pass the budget of the device
	// (set_resident_budget, default 1 GiB; no eviction) — the caller takes the glyf form.  *uploaded_bytes (may be NULL) is
	// raised by what this call put on the device (0: the copy was there).
	const vgsdf_font *resident_font(int lane, const ResidentTable &table, uint64_t *uploaded_bytes = nullptr) const;
	// the same font walked by the DEVICE from the face's loca and glyf tables (vgsdf_font_create_tables): same key (`serial` is
	// Face::resident_serial(), the table's), same budget through the call's own limit, same lifetime — whichever of the two calls
	// comes first makes the font and the other finds it.  nullptr: the device refused the face (*refused is set then, once per face
	// and device: the component budget, the bounds of the resident form, a device error) and the caller takes resident_font(),
	// which needs the host's table; or the font would pass the budget (*over_budget is set: the caller takes the glyf form).
	// *built: this call put the font on the device
	const vgsdf_font *font_from_tables(int lane, uint64_t serial, const FontTables &tables, uint64_t *uploaded_bytes, bool *refused,
	                                   bool *over_budget, bool *built) const;
	// font_from_tables for ALL faces of a font id in as few calls as their number and glyph ids allow (vgsdf_fonts_create_tables_within:
	// one count launch, one read-back, one emit launch per call).  Under the registry's lock for the whole of it, so two lanes of a
	// device never build a face twice.  A face is sent when its tables are ok, the registry has no font under (device, serial) and
	// it is not remembered as refused or as past the budget's room; what becomes of it is in outcomes[i] as font_from_tables says it
	// (uploaded: the font's device bytes), and the registry, the refused set and the sizes that did not fit are left as that
	// function would leave them, so that a font_from_tables of any of the faces behind this call finds its font, or goes the way it
	// went.  The call's own limit counts the stores' bytes and the registry their allocations (a quarter more): a font that the
	// registry's room does not take after all is freed again and remembered as one that did not fit.  *calls / *faces: the calls made, the faces sent
	struct TablesJob {
		uint64_t serial = 0;
		FontTables tables;
	};
	struct TablesOutcome {
		bool refused = false, over_budget = false, built = false;
		uint64_t uploaded = 0;
	};
	void fonts_from_tables(int lane, const std::vector<TablesJob> &faces, std::vector<TablesOutcome> &outcomes, uint64_t *calls, uint64_t *n_sent) const;
	// the same for the command store of a face (vgsdf_font_create_commands): same registry (the tables' serials come from one
	// sequence), same budget, no eviction.  nullptr: no command table, or over the budget — the caller goes on as without
	const vgsdf_font *command_font(int lane, const CommandTable &table, uint64_t *uploaded_bytes = nullptr) const;
	// the same store made on the device from a `CFF ` face's charstrings (vgsdf_font_create_charstrings) or, for a table with
	// cff2 set, from a `CFF2` face's and its blend sets (vgsdf_font_create_charstrings2): the key is the face's
	// command serial, so whichever of the two calls comes first makes the store and the other finds it.  nullptr: no charstring
	// table; the device refused the face (*refused is set then, once per face and device: a seac glyph, a glyph past the token
	// budget, a store past the bounds) and the caller takes command_font(), which needs the host's table; or the store would
	// pass the budget (*over_budget is set: command_font() would find the same store over the same budget, so the caller need
	// not build the host's table).  The size of a store that did not fit is kept, so the count pass is not run again while
	// it does not fit, and is once the budget has room for it
	const vgsdf_font *charstring_font(int lane, const CharstringTable &table, uint64_t *uploaded_bytes = nullptr, bool *refused = nullptr,
	                                  bool *over_budget = nullptr) const;
	// the same store made on the device from a placed glyf face's loca, glyf and gvar (vgsdf_font_create_gvar_within), under the
	// face's command serial: command_font() of the same face finds it.  refused / over_budget: as charstring_font says them; a
	// refusal is remembered per (device, serial), so the face goes the host's way once and is not tried again
	const vgsdf_font *gvar_font(int lane, uint64_t serial, const GvarTables &tables, uint64_t *uploaded_bytes, bool *refused, bool *over_budget) const;
	// gvar_font for ALL placed faces over ONE file's tables (the same loca, glyf and gvar; each its own coordinates and command
	// serial) in as few calls as their number allows (vgsdf_fonts_create_gvar_within: the tables uploaded once, one count launch,
	// the deltas and emit passes over all positions).  Shaped like fonts_from_tables: under the registry's lock for the whole of it;
	// a face is sent when its tables are ok, the registry has no font under (device, serial) and it is not remembered as refused or
	// as past the budget's room; outcomes[i], the registry, the refused set and the sizes that did not fit are left as gvar_font
	// would leave them, so that a gvar_font of any of the faces behind this call finds its store, or goes the way it went.
	// *calls / *n_sent: the calls made, the faces sent
	struct GvarJob {
		uint64_t serial = 0;
		GvarTables tables;
	};
	void gvar_fonts(int lane, const std::vector<GvarJob> &faces, std::vector<TablesOutcome> &outcomes, uint64_t *calls, uint64_t *n_sent) const;
	// charstring_font for ALL placed CFF2 faces over ONE file's charstrings (the same bytes, offsets and sets; each its own factors
	// and command serial) in as few calls as their number allows (vgsdf_fonts_create_charstrings2_within: the description uploaded
	// once, count and emit pass over all positions).  Shaped like gvar_fonts, the same registry protocol; what is remembered is
	// charstring_font's (DeviceBuilt charstrings), so that a charstring_font of any of the faces behind this call finds its store, or
	// goes the way it went.  A face whose table is not the first sent face's but for the factors is left to its own charstring_font
	struct Charstring2Job {
		uint64_t serial = 0;
		const CharstringTable *table = nullptr;
	};
	void charstring2_fonts(int lane, const std::vector<Charstring2Job> &faces, std::vector<TablesOutcome> &outcomes, uint64_t *calls,
	                       uint64_t *n_sent) const;
	// Resident families (vgsdf_family_create): the device copy of a font id's table code point -> (file, glyph id, advance,
	// scale, shift_x) over the device fonts of its files, one per (device, table serial, kind of store) in the registry of the
	// fonts — same budget, freed with the renderer, in front of the fonts.  A table rebuilt after a file was added has a new
	// serial and so a new family.  nullptr: over the budget
	struct FamilyArrays {
		uint64_t serial = 0;
		const std::vector<uint16_t> *code_point, *font_of, *glyph_id;
		const std::vector<uint32_t> *advance;
		const std::vector<double> *scale, *shift_x;
		uint32_t plane = 0; // code_point: the low halves of (plane << 16) | x (every table has its own serial, whatever its plane)
	};
	// kind: kFamilyGlyf / kFamilyCommands — every font of `fonts` of that kind — or kFamilyMixed: fonts of either kind, the family
	// made with the _mixed constructors (a third kind to the device, and a third key here)
	static constexpr int kFamilyGlyf = 0, kFamilyCommands = 1, kFamilyMixed = 2;
	const vgsdf_family *family(int lane, const FamilyArrays &table, const std::vector<const vgsdf_font *> &fonts, int kind,
	                           uint64_t *uploaded_bytes = nullptr) const;
	// the same family built by the DEVICE from the faces' cmap and hmtx tables (vgsdf_family_create_tables): same key (`serial`
	// stands for the table's), same budget, same lifetime.  *refused: the device has returned an error for this (device, serial),
	// 1 now or 2 earlier — the caller makes the family with family() instead; *built: this call put it on the device.  nullptr
	// without *refused: over the budget.  variation: empty (static faces only), or a record per face
	// (vgsdf_family_create_tables_var).  gvar: empty, or per face the description of one whose advances follow gvar's phantom
	// points, nullptr for every other (vgsdf_family_create_tables_gvar)
	const vgsdf_family *family_from_tables(int lane, uint64_t serial, const std::vector<vgsdf_face_tables> &tables,
	                                       const std::vector<const vgsdf_font *> &fonts, int kind, uint64_t *uploaded_bytes, int *refused,
	                                       bool *built, const std::vector<vgsdf_face_variation> &variation = {},
	                                       const std::vector<const vgsdf_font_gvar_desc *> &gvar = {}, uint32_t plane = 0) const;
	// (plane 1 .. 16: static faces only — variation and gvar empty — through vgsdf_family_create_tables_at)
	// vgsdf_family_tables_census over a font id's faces: bit p of *planes set where some block of plane p is listed.  false: not a
	// HIP renderer, or the call failed
	bool family_census(int lane, const std::vector<vgsdf_face_tables> &tables, uint32_t *planes) const;
	// family_from_tables for the families of ONE file's placed faces, a family of one face each (vgsdf_families_create_tables: the
	// tables uploaded once, one phantom pass, one count and one emit pass over all positions), in as few calls as their number
	// allows.  Shaped like gvar_fonts: under the registry's lock for the whole of it; a job is sent when its tables are ok and
	// those of the first job sent (the same cmap, hmtx and HVAR bytes, the same gvar or none), the registry has no family under
	// (device, serial, kind) and the key is not remembered as refused; outcomes[i], the registry and the refused set are left as
	// family_from_tables would leave them (a refused position, or every position of a call that failed, is remembered; a family
	// past the budget is freed and not remembered), so that a family_from_tables of any of the jobs behind this call finds its
	// family, or goes the way it went.  *calls / *n_families: the calls made, the families they made
	struct FamilyJob {
		uint64_t serial = 0;                  // of the family's shell
		const vgsdf_font *font = nullptr;     // the face's store on this device
		const FamilyTables *tables = nullptr; // the face's: hvar and region_scalars at its position
		GvarTables gvar;                      // ok: the face's advances follow gvar's phantom points
	};
	struct FamilyOutcome {
		bool refused = false, built = false;
		uint64_t uploaded = 0;
	};
	void families_from_tables(int lane, const std::vector<FamilyJob> &jobs, int kind, std::vector<FamilyOutcome> &outcomes, uint64_t *calls,
	                          uint64_t *n_families) const;
	// a family's code points and advances, read back (what a host that built no table names the glyphs of a ranges group by)
	void family_names(int lane, const vgsdf_family *family, std::vector<uint16_t> &code_point, std::vector<uint32_t> &advance) const;
	// a submission of code-point ranges of such families (n_glyphs: for the first capacity guess), and where its tasks'
	// rooms begin in the arena once it has been peeked at or waited for
	void submit_ranges(int lane, const vgsdf_outlines_ranges &batch, uint32_t n_glyphs, HostBuffer<uint8_t> &out, uint64_t *block_bytes) const;
	void task_extents(int lane, std::vector<uint64_t> &begin, uint32_t n_tasks) const;
	void set_resident_budget(uint64_t bytes_per_device);
	// Union outlines (rule U; off by default): every Hip route renders the boundary of a glyph's filled set
	// instead of its segments — render_batch / render_packed go upload, vgsdf_batch_union, launch, download, and the device
	// front-end's submissions go without a destination (no raster behind the plan), vgsdf_outlines_union, vgsdf_outlines_render
	// in wait_outlines.  Dummy ignores it.  Reaches the peers of a multi-device renderer.  FontManager sets it for its runs
	// (render_glyphs, render_blocks) and takes it back afterwards: the switch and the counts below are the RENDERER's, so a
	// renderer serves one manager's run at a time — two managers that render on one renderer from two threads at once would
	// switch each other's run and share the counts (runs one after the other, with any switches, are fine).
	void set_union_outlines(bool on) const;
	bool union_outlines() const { return union_outlines_.load(); }
	// glyphs the union pass has seen since the last call, by state {identity, rebuilt, over the limit, non-finite}; resets them
	void take_union_stats(uint64_t by_state[4]) const;
	uint64_t resident_bytes(int device) const; // what the renderer's resident fonts occupy on a device
	void wait_outlines(int lane, std::vector<vgsdf_rect> &rects, HostBuffer<uint8_t> &out, uint64_t &out_bytes,
	                   uint64_t &n_segments, uint32_t n_glyphs, std::vector<uint64_t> *pbf_at = nullptr) const;
	// Between the two: the front-end's results as soon as they are on the host, while the raster is still running
	// (vgsdf_outlines_peek).  Returns true when the raster is storing the bitmaps straight into `out` as it stands, so
	// that the caller may write the bytes between them (in-place PBF assembly) right away.
	bool peek_outlines(int lane, std::vector<vgsdf_rect> &rects, uint64_t &out_bytes, uint32_t n_glyphs,
	                   std::vector<uint64_t> *pbf_at = nullptr) const;

	// Device half for a packed batch: fills out[batch.out_bytes()].  Hip: one
	// vgsdf_render_batch call; Dummy: zeros (renderer_dummy.rs).  Throws std::runtime_error.
	void render_batch(const GlyphBatch &batch, uint8_t *out) const;
	// Same for a packed (page-locked) batch; pixels land in batch.out.
	void render_packed(PackedBatch &batch) const;

	// renderer.rs:103 — per-glyph API kept for drop-in parity (a batch of one).
	std::optional<PbfGlyph> render_glyph(const Face &face, uint32_t index) const;

	vgsdf_ctx *ctx() const { return ctx_; }
	std::mutex &ctx_mutex() const { return mu_; }

private:
	Renderer() = default;
	Mode mode_ = Mode::Dummy;
	int device_ = 0;
	vgsdf_ctx *ctx_ = nullptr;
	mutable std::mutex mu_; // vgsdf_ctx is single-threaded
	mutable vgsdf_ctx *ctx2_ = nullptr; // lane 1 of the two-deep pipeline (created on first use)
	mutable std::mutex lane_mu_[2];     // held from submit_outlines to wait_outlines
	vgsdf_ctx *lane_ctx(int lane) const;
	mutable std::atomic<bool> union_outlines_{false};
	mutable std::atomic<uint64_t> union_seen_[4] = {};
	void count_union_states(const std::vector<uint8_t> &state) const;
	// vgsdf_render_batch, or with union outlines its four steps around vgsdf_batch_union; under mu_
	void render_view(const vgsdf_batch &v, uint8_t *out) const;
	// what the submit_outlines overloads share: the lane held from here to wait_outlines (released when this throws), the first
	// capacity guess for `out`, the context's lock around the C call `submit` (`name`: for the error)
	template <class Batch>
	void submit_on_lane(int lane, const Batch &v, HostBuffer<uint8_t> &out, int (*submit)(vgsdf_ctx *, const Batch *, uint8_t *, size_t),
	                    const char *name, uint64_t *block_bytes = nullptr) const;
	// a resident font or family made by the C call `create` through the lane's context, under its lock; throws what the call says (`name`: for the error)
	template <class Desc, class Made> Made *create_resident(int lane, int (*create)(vgsdf_ctx *, const Desc *, Made **), const Desc &d, const char *name) const;
	std::vector<std::shared_ptr<Renderer>> peers_; // device lanes 1 .. N-1 of a multi-device renderer
	struct ResidentFonts { // of a renderer and its peers
		std::mutex mu;
		std::map<std::pair<int, uint64_t>, vgsdf_font *> fonts; // (device, the face's serial number) -> its copy there
		// (device, table serial, kind of stores) -> the family.  A font id's families of different PLANES are different tables, each
		// with a serial of its own, so the serial stands for the plane as well
		std::map<std::tuple<int, uint64_t, int>, vgsdf_family *> families;
		std::map<int, uint64_t> bytes;                          // per device
		std::set<std::tuple<int, uint64_t, int>> refused_family_tables; // the key of `families`: the device has refused to build the table
		// What the registry remembers of the faces one kind of DEVICE-BUILT font was asked for and did not get, by (device, serial):
		// those the device's builder has refused (they go the host's way, once) and the bytes of those that passed the budget (the
		// count pass is not run again while they do not fit, and is once the budget has room for them)
		struct DeviceBuilt {
			using Key = std::pair<int, uint64_t>;
			enum Known { kNothing, kRefused, kUnfit };
			std::set<Key> refused;
			std::map<Key, uint64_t> unfit;
			Known known(const Key &key, uint64_t room) const // refused, or known not to fit this room?
			{
				if (refused.count(key))
					return kRefused;
				const auto it = unfit.find(key);
				return it != unfit.end() && it->second > room ? kUnfit : kNothing;
			}
			void remember_refused(const Key &key) { refused.insert(key); }
			void remember_unfit(const Key &key, uint64_t bytes) { unfit[key] = bytes; }
			void fitted(const Key &key) { unfit.erase(key); }
			void clear() { refused.clear(), unfit.clear(); }
		};
		DeviceBuilt glyf_tables, charstrings, gvar; // font_from_tables / fonts_from_tables, charstring_font, gvar_font / gvar_fonts
		uint64_t budget = 1ull << 30;
		void clear() // (the owner has freed the fonts and families)
		{
			families.clear(), fonts.clear(), bytes.clear(), refused_family_tables.clear();
			glyf_tables.clear(), charstrings.clear(), gvar.clear();
		}
		// the frame of resident_font() .. family_from_tables() (under `mu`): what the registry holds under a key, the budget a device has left, and a new
		// font or family of `got` device bytes taken in and accounted (the key's first member is the device)
		template <class Map, class Key> static typename Map::mapped_type find(const Map &map, const Key &key) { const auto it = map.find(key); return it != map.end() ? it->second : nullptr; }
		uint64_t room(int device) { return budget > bytes[device] ? budget - bytes[device] : 0; }
		template <class Map, class Key> typename Map::mapped_type keep(Map &map, const Key &key, typename Map::mapped_type made, uint64_t got, uint64_t *uploaded_bytes)
		{
			map.emplace(key, made);
			bytes[std::get<0>(key)] += got;
			if (uploaded_bytes)
				*uploaded_bytes += got;
			return made;
		}
	};
	// The protocol of font_from_tables(), charstring_font() and gvar_font(), under the registry's lock: found? refused before? known not
	// to fit the room?  Then build(context, room, &font, &bytes) makes the C call under the context's lock: refused — VGSDF_E_GLYF, or
	// any failure where `throws_as` is NULL; another failure throws under that name —, over the budget as it stands (no font), or kept.
	// The three out-parameters may be NULL
	template <class Build>
	const vgsdf_font *device_built_font(int lane, ResidentFonts::DeviceBuilt &kind, uint64_t serial, const char *throws_as, Build build,
	                                    uint64_t *uploaded_bytes, bool *refused, bool *over_budget, bool *built) const;
	// ... and what fonts_from_tables() and gvar_fonts() make of one batched call's made[], status[] and needed[] for the faces `sent`
	// (failed: the call itself did, every face counts as refused): outcomes[] and the registry as that protocol leaves them
	template <class Job>
	void settle_batch(ResidentFonts::DeviceBuilt &kind, vgsdf_ctx *c, bool failed, const std::vector<Job> &faces, const std::vector<size_t> &sent,
	                  std::vector<vgsdf_font *> &made, const std::vector<int> &status, const std::vector<uint64_t> &needed,
	                  std::vector<TablesOutcome> &outcomes) const;
	std::shared_ptr<ResidentFonts> resident_ = std::make_shared<ResidentFonts>();
	bool owns_resident_ = true; // (a peer shares its primary's table and leaves the freeing to it)
};

} // namespace vg
