// font_manager.hpp — host mirror of the reference's orchestration layer for the render
// path, with the rayon block loop replaced by a GPU batch dispatcher.
//
//   FontFileEntry                       /root/reference/src/font/file_entry.rs:16-56
//   FontWrapper::{add_file,get_blocks}  src/font/wrapper.rs:21-76
//   GlyphBlock::{set_glyph_font,render,filename}   src/font/glyph_block.rs:10-90
//   FontManager::{new,add_font_with_name,render_glyphs}  src/font/manager.rs:18-125
//   name_to_id                          manager.rs:141-147
//   WriterTrait                         src/writer/mod.rs:10-19
//
//   FontManager::{add_path,add_paths}  manager.rs:39-61;  scan  src/commands/recurse.rs:104-133
//   write_index_json / write_families_json   manager.rs:128-138 (index_files.hpp)
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>
#include <deque>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "font_name.hpp"
#include "renderer.hpp"
#include "thread_pool.hpp"

namespace vg {

constexpr uint32_t GLYPH_BLOCK_SIZE = 256; // glyph_block.rs:7

// Sink for rendered files (writer/mod.rs:10-19).  write_file may be called from the
// dispatcher thread only (the reference serialises writers behind a Mutex, manager.rs:102).
struct Writer {
	virtual ~Writer() = default;
	virtual void write_directory(const std::string &path) = 0;
	virtual void write_file(const std::string &path, const std::vector<uint8_t> &data) = 0;
	// the same for bytes that live in someone else's buffer (a block assembled in place in the device's output arena):
	// sinks that can take a pointer override it and save the copy
	virtual void write_bytes(const std::string &path, const uint8_t *data, size_t len) { write_file(path, std::vector<uint8_t>(data, data + len)); }
	// ... and for a file whose bytes lie in several places (a block whose glyphs were rendered by several device lanes: its
	// header and the lanes' runs of entries): sinks that stream override it; the default joins the pieces first
	using Piece = std::pair<const uint8_t *, size_t>;
	virtual void write_gather(const std::string &path, const Piece *pieces, size_t n)
	{
		std::vector<uint8_t> all;
		for (size_t i = 0; i < n; i++)
			all.insert(all.end(), pieces[i].first, pieces[i].first + pieces[i].second);
		write_bytes(path, all.data(), all.size());
	}
	virtual void finish() {} // writer/mod.rs:71-77
};

// file_entry.rs: owns the bytes, the parsed face and the cmap coverage
class FontFileEntry {
public:
	// coords: the face at that position (Face::parse_at) instead of as parsed
	// (gvar_advances: Face::parse_at's — a placed glyf face without HVAR takes its advances from gvar's phantom points)
	static std::unique_ptr<FontFileEntry> create(std::vector<uint8_t> data, std::string *err, const std::vector<int16_t> *coords = nullptr,
	                                             bool gvar_advances = false);
	// the same over bytes that several entries share (the named instances of one file); ps_name: the PostScript name the metadata
	// is parsed from instead of the file's name id 6
	static std::unique_ptr<FontFileEntry> create(std::shared_ptr<const std::vector<uint8_t>> data, std::string *err,
	                                             const std::vector<int16_t> *coords, const std::string *ps_name, bool gvar_advances = false);
	const Face &face() const { return face_; }
	const std::vector<uint32_t> &codepoints() const { return codepoints_; } // metadata.rs:105-119
	const FontMetadata &metadata() const { return metadata_; }                // metadata.rs:89-103

private:
	std::shared_ptr<const std::vector<uint8_t>> data_;
	Face face_;
	std::vector<uint32_t> codepoints_;
	FontMetadata metadata_;
};

// glyph_block.rs:10-16 — which file renders each of the 256 code points of a range
struct GlyphBlock {
	uint32_t start_index = 0;
	std::array<const FontFileEntry *, GLYPH_BLOCK_SIZE> glyphs{}; // nullptr = unmapped
	uint32_t count = 0;
	bool all_glyf = true; // every glyph of the block comes from a file with `glyf` outlines (the device can decode them)

	// glyph_block.rs:34-36: first provider wins
	void set_glyph_font(uint8_t char_index, const FontFileEntry *font)
	{
		if (!glyphs[char_index]) {
			glyphs[char_index] = font;
			count++;
			all_glyf = all_glyf && font->face().has_glyf_form();
		}
	}
	size_t len() const { return count; }
	bool is_empty() const { return count == 0; }
	const std::string &range() const; // glyph_block.rs:53-59 (the 256 strings of the BMP blocks are built once)
	std::string filename() const { return range() + ".pbf"; } // :85-87
	// "<font>/<range>.pbf" into a caller-owned string (its capacity is reused: one task of a run after the other)
	void path_into(const std::string &font, std::string &out) const
	{
		out.assign(font);
		out.push_back('/');
		out += range();
		out += ".pbf";
	}

	// Host half of GlyphBlock::render (glyph_block.rs:72-77), glyphs in ascending id;
	// [ci0, ci1) restricts it to a sub-range of the block's 256 code points.
	void prepare(TessScratch &scratch, GlyphBatch &batch, uint32_t ci0 = 0, uint32_t ci1 = GLYPH_BLOCK_SIZE) const;
	// glyph_block.rs:69-80 complete (one block through the renderer)
	std::vector<uint8_t> render(const std::string &font_name, const Renderer &renderer) const;
};

// wrapper.rs:15-19
class FontWrapper {
public:
	void add_file(std::unique_ptr<FontFileEntry> f)
	{
		files_.push_back(std::move(f));
		blocks_valid_ = false;
	}
	bool add_paths(const std::vector<std::string> &paths, std::string *err); // wrapper.rs:31-39
	const std::vector<std::unique_ptr<FontFileEntry>> &files() const { return files_; }
	// wrapper.rs:53-76: always the 256 blocks of the BMP, empty ones included; with set_supplementary(true) one block more per
	// POPULATED range of 256 code points above U+FFFF, ascending behind them (empty ones are not listed: 4096 empty files per font
	// serve nobody); first provider wins there as in the BMP
	std::vector<GlyphBlock> get_blocks() const;
	void set_supplementary(bool on)
	{
		if (supplementary_ != on)
			blocks_valid_ = false;
		supplementary_ = on;
	}
	// the block that starts at `start` in a table get_blocks (or a rank's share of it) made; nullptr: none
	static const GlyphBlock *find_block(const std::vector<GlyphBlock> &blocks, uint32_t start);
	// the same table, built once per set of files (0.5 MiB per font: rebuilding it for every
	// render_glyphs call was 7 % of an end-to-end run); valid until the next add_file / add_paths
	const std::vector<GlyphBlock> &blocks() const
	{
		if (!blocks_valid_) {
			blocks_ = get_blocks();
			blocks_valid_ = true;
		}
		return blocks_;
	}

private:
	std::vector<std::unique_ptr<FontFileEntry>> files_;
	mutable std::vector<GlyphBlock> blocks_;
	mutable bool blocks_valid_ = false;
	bool supplementary_ = false;
};
constexpr uint32_t kBmpBlocks = 0x10000 / GLYPH_BLOCK_SIZE; // wrapper.rs:55

// Glyph-level shard of one font over `world` ranks: every mapped code point <= 0xFFFF has an
// owner; costs are estimates of w*h*N (bitmap area x segment count) computed from the recorded outline
// commands, identical on every rank, so all ranks derive the same assignment without talking to each other.
struct GlyphShard {
	uint32_t world = 1;
	std::vector<uint8_t> owner; // [65536]: rank that renders the code point, 0xFF = not mapped by the font
	std::vector<double> cost;   // [65536]: estimated cost (0 for unmapped)
	std::vector<double> load;   // [world]: sum of estimated costs per rank
};

struct RenderTimings {
	double tessellate_s = 0, pack_s = 0, device_s = 0, encode_s = 0, write_s = 0, total_s = 0;
	uint64_t blocks = 0, glyphs = 0, rasters = 0, pixels = 0, segments = 0, pbf_bytes = 0;
	uint64_t glyf_groups = 0, glyf_fallbacks = 0; // device front-end: groups decoded from `glyf` arrays / re-recorded on the host
	uint64_t fe_groups = 0, fe_max_group_glyphs = 0; // the dispatcher's groups that held glyphs (one submission each), the largest's glyphs
	// resident fonts: groups submitted by (font, glyph id), faces uploaded during the run and their bytes on the device, bytes of
	// the submissions' upload blocks
	uint64_t resident_groups = 0, resident_fonts_uploaded = 0, resident_font_bytes = 0, resident_block_bytes = 0;
	// the same for groups submitted by name against command stores (set_resident_commands)
	uint64_t command_groups = 0, command_fonts_uploaded = 0, command_font_bytes = 0, command_block_bytes = 0;
	// groups submitted as code-point ranges of resident families (counted here and not above), families put on a device, their
	// bytes there, bytes of those submissions' upload blocks
	uint64_t family_groups = 0, families_uploaded = 0, family_bytes = 0, family_block_bytes = 0;
	// command stores the device decoded from charstrings (set_charstrings_on_device; counted among command_fonts_uploaded too),
	// their bytes, and faces it refused, whose stores were built from the host reader's table instead
	uint64_t charstring_fonts_decoded = 0, charstring_font_bytes = 0, charstring_fallbacks = 0;
	// families whose tables the device built from cmap and hmtx (set_family_tables_on_device; counted among families_uploaded
	// too), and font ids whose description refused or whose build the device refused: their families were made the host's way
	uint64_t family_tables_built = 0, family_table_fallbacks = 0;
	// glyf-kind fonts the device walked from loca and glyf (set_glyf_tables_on_device; counted among resident_fonts_uploaded too),
	// their bytes, and faces whose build the device refused: their fonts were made from the host's table instead
	uint64_t glyf_tables_built = 0, glyf_table_bytes = 0, glyf_table_fallbacks = 0;
	// ... and, with set_glyf_tables_batched, the calls that built them (one per font id whose faces needed building) and the faces sent
	uint64_t glyf_table_batch_calls = 0, glyf_table_batch_faces = 0;
	// groups submitted against stores of BOTH kinds (set_mixed_stores; counted here and in none of the group counters above), the
	// glyf stores and the command stores those groups named, bytes of their upload blocks
	uint64_t mixed_groups = 0, mixed_glyf_fonts = 0, mixed_command_fonts = 0, mixed_block_bytes = 0;
	// command stores the device built from a placed glyf face's loca, glyf and gvar (set_gvar_on_device; counted among
	// command_fonts_uploaded too), their bytes, and faces it refused, whose stores were built from the host reader's table instead
	uint64_t gvar_fonts_built = 0, gvar_font_bytes = 0, gvar_fallbacks = 0;
	// ... and, with set_gvar_batched, the calls that built them (one per group of faces over the same bytes) and the faces sent
	uint64_t gvar_batch_calls = 0, gvar_batch_faces = 0;
	// with set_charstrings_batched: the calls that built CFF2 instances' stores (one per group of faces over the same bytes), the faces sent
	uint64_t charstring_batch_calls = 0, charstring_batch_faces = 0;
	// families with a face whose advances follow gvar's phantom points (set_gvar_advances) that the device built, the phantom pass
	// included (set_family_tables_on_device; counted among family_tables_built too), and those it refused, whose tables came from
	// the host reader instead (counted among family_table_fallbacks too)
	uint64_t gvar_advance_builds = 0, gvar_advance_fallbacks = 0;
	// with set_family_tables_batched: the calls that built the family tables of the instances of one file in one device build
	// (one per group of faces over the same bytes and device lane) and the families they made (counted among family_tables_built too)
	uint64_t family_batch_calls = 0, family_batch_families = 0;
	// supplementary planes: census calls (one per font id whose supplementary family the device is to build), supplementary
	// families the device built (vgsdf_family_create_tables_at; counted among family_tables_built too), those the host stated
	// (vgsdf_family_create_at: a font id with a placed face, the switch off, a refusal), and the planes 1 .. 16 either kind was
	// made for, bit p for plane p
	uint64_t family_census_calls = 0, plane_families_built = 0, plane_families_stated = 0, plane_family_planes = 0;

	// The timings of a device lane of a multi-lane run folded into the run's: the lanes work side by side, so a phase takes as
	// long as the slowest lane's; counters add up.  (blocks, pbf_bytes, write_s and total_s are the run's own: it writes the files.)
	void absorb_lane(const RenderTimings &lane)
	{
		tessellate_s = std::max(tessellate_s, lane.tessellate_s);
		pack_s = std::max(pack_s, lane.pack_s);
		device_s = std::max(device_s, lane.device_s);
		encode_s = std::max(encode_s, lane.encode_s);
		glyphs += lane.glyphs, rasters += lane.rasters, pixels += lane.pixels, segments += lane.segments;
		glyf_groups += lane.glyf_groups, glyf_fallbacks += lane.glyf_fallbacks;
		fe_groups += lane.fe_groups;
		fe_max_group_glyphs = std::max(fe_max_group_glyphs, lane.fe_max_group_glyphs);
		resident_groups += lane.resident_groups, resident_block_bytes += lane.resident_block_bytes;
		command_groups += lane.command_groups, command_block_bytes += lane.command_block_bytes;
		family_groups += lane.family_groups, family_block_bytes += lane.family_block_bytes;
		mixed_groups += lane.mixed_groups, mixed_glyf_fonts += lane.mixed_glyf_fonts, mixed_command_fonts += lane.mixed_command_fonts;
		mixed_block_bytes += lane.mixed_block_bytes;
		add_uploads(lane);
	}
	// what `counts` says was put on a device — stores, families, decoded charstrings — added to these
	void add_uploads(const RenderTimings &counts)
	{
		resident_fonts_uploaded += counts.resident_fonts_uploaded, resident_font_bytes += counts.resident_font_bytes;
		command_fonts_uploaded += counts.command_fonts_uploaded, command_font_bytes += counts.command_font_bytes;
		families_uploaded += counts.families_uploaded, family_bytes += counts.family_bytes;
		charstring_fonts_decoded += counts.charstring_fonts_decoded, charstring_font_bytes += counts.charstring_font_bytes;
		charstring_fallbacks += counts.charstring_fallbacks;
		family_tables_built += counts.family_tables_built, family_table_fallbacks += counts.family_table_fallbacks;
		glyf_tables_built += counts.glyf_tables_built, glyf_table_bytes += counts.glyf_table_bytes, glyf_table_fallbacks += counts.glyf_table_fallbacks;
		glyf_table_batch_calls += counts.glyf_table_batch_calls, glyf_table_batch_faces += counts.glyf_table_batch_faces;
		gvar_fonts_built += counts.gvar_fonts_built, gvar_font_bytes += counts.gvar_font_bytes, gvar_fallbacks += counts.gvar_fallbacks;
		gvar_batch_calls += counts.gvar_batch_calls, gvar_batch_faces += counts.gvar_batch_faces;
		charstring_batch_calls += counts.charstring_batch_calls, charstring_batch_faces += counts.charstring_batch_faces;
		gvar_advance_builds += counts.gvar_advance_builds, gvar_advance_fallbacks += counts.gvar_advance_fallbacks;
		family_batch_calls += counts.family_batch_calls, family_batch_families += counts.family_batch_families;
		family_census_calls += counts.family_census_calls, plane_families_built += counts.plane_families_built;
		plane_families_stated += counts.plane_families_stated, plane_family_planes |= counts.plane_family_planes;
	}
};
// (a field added above belongs in one of the two folds, or in the comment of the first)
static_assert(sizeof(RenderTimings) == 6 * sizeof(double) + 51 * sizeof(uint64_t), "RenderTimings has a field its folds do not know");

class FontManager {
public:
	explicit FontManager(bool parallel) : parallel_(parallel) {} // manager.rs:28-33
	~FontManager();

	// manager.rs:66-75
	bool add_font_with_name(const std::string &name, const std::vector<std::string> &sources, std::string *err);
	bool add_font_data(const std::string &name, std::vector<uint8_t> data, std::string *err);
	// A variable file at a position of its design space, under a name of the caller's: a file like any other from here on (the
	// same name merges, another name is another font id; every instance is a Face of its own with its own serials, so no two
	// share a store on a device).  Normalised: final coordinates, one per fvar axis.  The other form takes user-space values by
	// axis tag (4 bytes each), axes not named stay at their default; values are normalised (normalize_axis_value) and sent
	// through the file's avar (apply_avar).  false: an unknown tag, a tag twice, a value that is not finite, or what
	// Face::parse_at refuses.
	bool add_font_instance_normalized(const std::string &name, std::vector<uint8_t> data, const std::vector<int16_t> &coords, std::string *err);
	bool add_font_instance(const std::string &name, std::vector<uint8_t> data, const std::vector<std::array<char, 4>> &tags,
	                       const std::vector<float> &values, std::string *err);
	// Every named instance of the file's fvar as a font id of its own, by add_font_instance's rules (normalize_axis_value, apply_avar,
	// what Face::parse_at refuses); all instances share ONE copy of the bytes.  The id of an instance: parse_font_name(family,
	// ps_name) -> generate_name -> name_to_id, with ps_name by named_instance_ps_names (ttf_face.hpp); two instances that arrive at
	// one id merge like any files of one id.  ids: the font id of every record, in the table's order.  false, nothing added: no
	// readable fvar, no instance record, or a refusal of add_font_instance's (a glyf face without a readable gvar ...).
	bool add_font_named_instances(std::vector<uint8_t> data, std::vector<std::string> &ids, std::string *err);
	// add_path and scan treat a variable file that has instance records as add_font_named_instances does (default off: as any file)
	void set_scan_named_instances(bool on) { scan_named_instances_ = on; }
	// manager.rs:39-53: the file's own name table decides the font id (family + width + weight + style
	// through parse_font_name / generate_name / name_to_id); files with the same id merge, in call order
	bool add_path(const std::string &path, std::string *err);
	bool add_paths(const std::vector<std::string> &paths, std::string *err); // manager.rs:56-61
	// recurse.rs:104-133: a file named *.ttf / *.otf is added; a directory with a fonts.json is read
	// through it ([{name, sources[]}], sources relative to that directory) and NOT descended into; any
	// other directory is walked.  The reference walks in fs::read_dir order (unspecified, so the
	// first-provider-wins merge depends on the file system); here entries are visited in ascending
	// byte order of their names, the canonical order of SURVEY.md §8a.
	bool scan(const std::string &path, std::string *err);
	// manager.rs:128-138
	void write_index_json(Writer &writer) const;
	void write_families_json(Writer &writer) const;

	// manager.rs:81-125.  Host threads tessellate blocks into SoA batches, the GPU renders
	// them, blocks are PBF-encoded and handed to the writer in task order.  Throws
	// std::runtime_error on failure (first error aborts, like try_for_each).
	void render_glyphs(Writer &writer, const Renderer &renderer);
	// Same, restricted to the given block start indices of one font (a rank's shard of the
	// (font, block) task list; blocks are independent: manager.rs:86-97).
	void render_blocks(Writer &writer, const Renderer &renderer, const std::string &font_id,
	                   const std::vector<uint32_t> &block_starts);

	// ---- glyph-level sharding (the reference's unit is the (font, block) task, manager.rs:86-97; 45 non-empty,
	// very unequal blocks do not balance over 8 GPUs, single glyphs do) ----
	// Longest-processing-time-first assignment of the font's glyphs to `world` ranks by estimated cost.
	bool shard_glyphs(const std::string &font_id, uint32_t world, GlyphShard &out, std::string *err) const;
	// From now on render_glyphs / render_blocks / build_batch / record_outlines see only the glyphs rank `rank`
	// owns (every block is still emitted: its PBF then holds this rank's glyphs only, a "partial" that
	// merge_pbf_partials() combines with the other ranks').  world <= 1 switches sharding off.
	void set_glyph_shard(uint32_t rank, uint32_t world);

	// Host stage only: every rasterised glyph of one font, blocks in ascending order (the
	// batch a bench/test keeps resident in HBM).  ids[i] = code point of rasterised glyph i.
	bool build_batch(const std::string &font_id, PackedBatch &out, std::vector<uint32_t> &ids, uint32_t &n_jobs,
	                 std::string *err);

	// Host half of the device front-end for every glyph of one font (ascending code point,
	// first provider wins): what vgsdf_outlines_prepare is fed.
	bool record_outlines(const std::string &font_id, OutlineBatch &out, std::string *err) const;

	const std::map<std::string, FontWrapper> &fonts() const { return parent_ ? parent_->fonts_ : fonts_; }
	const RenderTimings &last_timings() const { return timings_; }
	// {blocks, glyphs, pixels} of the last multi-device render_glyphs, as vgsdf_reduce_counters summed them over the
	// device lanes (all zero after a single-device run: there is nothing to reduce)
	const uint64_t *last_reduced_counters() const { return reduced_; }
	void set_threads(unsigned n) { threads_ = n; }
	void set_batch_blocks(unsigned n)
	{
		batch_blocks_ = n ? n : 1;
		batch_blocks_set_ = true;
	}
	// true: flatten / close / scale / bbox on the GPU (device front-end, HIP renderer only);
	// false: host tessellation.  Both produce identical bytes.
	void set_device_front_end(bool on) { device_front_end_ = on; }
	bool device_front_end() const { return device_front_end_; }
	// true: union outlines (rule U) — render_glyphs and render_blocks of this manager hand the switch to their
	// renderer for the run (Renderer::set_union_outlines), on either route; the bitmaps are then deliberately NOT the reference's.  Off by default;
	// the dummy renderer ignores it.  Metrics, advances and PBF framing do not change.
	void set_union_outlines(bool on) { union_outlines_ = on; }
	bool union_outlines() const { return union_outlines_; }
	// glyphs the union pass has seen in this manager's runs: {identity, rebuilt, passed through over the limit, passed through
	// with a non-finite coordinate}
	const uint64_t *union_stats() const { return union_stats_; }
	// true (default): with the device front-end the blocks are assembled IN PLACE — the raster stores every bitmap where
	// the finished PBF has it and the host writes the ~20 bytes around it; false: bitmaps packed back to back, blocks
	// encoded afterwards (one more copy of every bitmap).  Same bytes either way.
	void set_in_place_pbf(bool on) { in_place_pbf_ = on; }
	// glyf fonts through the device front-end: true (default; VG_GLYF_ON_DEVICE=0 in the environment changes it) = the
	// device decodes the glyphs' `glyf` arrays, false = the host's reader records the callbacks.  Same bytes either way.
	void set_glyf_on_device(bool on) { glyf_on_device_ = on; }
	// Resident fonts (default off): a group whose faces all have `glyf` outlines and a resident form is submitted by
	// (font, glyph id) against the renderer's device copies of the faces (uploaded on first use); everything else as ever
	void set_resident_fonts(bool on) { resident_fonts_ = on; }
	// Command stores (default 0, independent of the switch above).  1: a group that cannot take a glyf form — a face without
	// `glyf` outlines, a font the device's decoder or the batch bounds have refused — goes by (font, glyph id) against
	// command stores of all its faces instead of through the host's reader; groups that can take a glyf form are untouched.
	// 2: every group goes that way, `glyf` faces included (the A/B lever).  A store that does not fit the renderer's
	// budget sends its groups the way they go with 0.
	void set_resident_commands(int mode) { resident_commands_ = mode < 0 || mode > 2 ? 0 : mode; }
	// Mixed stores (default off; has an effect only with the device's glyf decoder, resident fonts and set_resident_commands(1)): a
	// group that cannot take a glyf form because SOME glyph comes from a file without `glyf` outlines no longer sends every file of
	// its font ids to the command stores.  Stores go per FILE — a `glyf` file whose glyf store can be made gets that one, every
	// other file a command store — and the group is submitted against both kinds at once (by name, or as ranges of mixed
	// families).  A group none of whose files gets a glyf store goes to the command forms as without the switch.
	void set_mixed_stores(bool on) { mixed_stores_ = on; }
	// ... and whether the switches are such that it has an effect
	bool mixes() const { return mixed_stores_ && glyf_on_device_ && resident_fonts_ && resident_commands_ == 1; }
	// Command stores of `CFF ` version 1 faces decoded on the device from the charstrings (vgsdf_font_create_charstrings) instead
	// of uploaded from command_table(); a face the device refuses falls back.  Default off.  The stores' bytes are the same.
	// 2: CFF2 faces too (vgsdf_font_create_charstrings2, with the reader's blend factors: those of the face's position, the
	// default one unless the file was added by add_font_instance).
	void set_charstrings_on_device(int mode) { charstrings_on_device_ = mode < 0 || mode > 2 ? 0 : mode; }
	const CharstringTable *charstring_table(const std::string &font_id, size_t file_index, std::string *err) const;
	const CharstringTable *charstring2_table(const std::string &font_id, size_t file_index, std::string *err) const;
	// what the last preload_resident_fonts built: its uploads are counted here, not in the timings of a render
	const RenderTimings &last_preload_counts() const { return preload_counts_; }
	// Resident families (default off): a group that would be recorded glyph by glyph against resident fonts or command stores
	// (the two switches above) is submitted as code-point ranges of its font ids' families instead — one task per (font, block),
	// one per run of code points for a block the hybrid lane plan has split — and the device writes the PBF entries; recording
	// is O(tasks).  With glyph sharding on (set_glyph_shard, lane form 0) groups go by glyph names as without the switch
	void set_resident_families(bool on) { resident_families_ = on; }
	// Supplementary planes (default off): every font id's block table lists, behind the 256 blocks of the BMP, one block per
	// populated range of 256 code points above U+FFFF (FontWrapper::get_blocks), and render_glyphs / render_blocks write their
	// files like any other.  A supplementary block is never split: under set_glyph_shard it belongs whole to rank
	// (start / 256) % world, in a multi-device run to that lane.  The forms that name glyphs take such a block as any other; the
	// ranges forms name the font id's family of the block's PLANE: built by the device for a static font id with
	// set_family_tables_on_device (planes chosen by one census per font id), from family_table(font_id, err, plane) otherwise.
	// With the switch off every byte stays what it is.
	void set_supplementary_planes(bool on);
	bool supplementary_planes() const { return supplementary_planes_; }
	// Family tables on the device (default off): a resident family's table is built by the device from the faces' cmap and hmtx
	// tables (Face::family_tables, vgsdf_family_create_tables) and family_table() below is not built for the font id; a font id
	// whose description refuses, or whose build the device refuses, gets its family the host's way (remembered).  Same table bytes.
	// A file at a position (add_font_instance) hands its HVAR and the factors of its regions over as well
	// (vgsdf_family_create_tables_var): the device adds the advance's offset where the host's reader would.
	void set_family_tables_on_device(bool on) { family_tables_on_device_ = on; }
	// Glyf tables on the device (default off): wherever the renderer makes a glyf-kind resident font — glyph-named groups, the
	// families, preload_resident_fonts — the DEVICE walks the face's loca and glyf (Face::font_tables, vgsdf_font_create_tables)
	// and Face::resident_table() is not built for the face; a face whose build the device refuses gets its font from the host's
	// table (remembered per face and device).  Same leaves, same output.
	void set_glyf_tables_on_device(bool on) { glyf_tables_on_device_ = on; }
	// a placed glyf face's command store is built on the device from loca, glyf and gvar (Renderer::gvar_font); a face the device
	// refuses gets its store from the host reader's table, as with the switch off
	void set_gvar_on_device(bool on) { gvar_on_device_ = on; }
	// with set_gvar_on_device: the stores of ALL placed glyf faces over the same bytes (add_font_named_instances) that the lane's
	// device has yet to build, in one call when the first of them is asked for (Renderer::gvar_fonts)
	void set_gvar_batched(bool on) { gvar_batched_ = on; }
	// with set_charstrings_on_device(2): the stores of ALL placed CFF2 faces over the same bytes (add_font_named_instances) that the
	// lane's device has yet to build, in one call when the first of them is asked for (Renderer::charstring2_fonts)
	void set_charstrings_batched(bool on) { charstrings_batched_ = on; }
	// The batched description (vgsdf_fonts_create_charstrings2) of the instance group the ONE file of `font_id` belongs to, in the
	// group's order: the first face's charstring2_table() and the factors of every face, one behind the other (views that stay
	// while the manager holds the fonts).  false, *err: where charstring2_table(font_id, 0) fails, a font id not in a group, a face
	// of the group without such a table, or faces that disagree in anything but the factors
	struct Charstring2Group {
		const CharstringTable *first = nullptr;
		const float *factors = nullptr;
		uint32_t n_positions = 0;
	};
	bool charstring2_group(const std::string &font_id, Charstring2Group &out, std::string *err) const;
	// with set_family_tables_on_device: when the family of a font id whose ONE file is a placed face that shares its bytes with
	// other placed faces (add_font_named_instances, glyf + gvar and CFF2 alike) is asked for, the family tables of ALL such font
	// ids of that group that the lane's device lacks are built in one call (Renderer::families_from_tables: the tables uploaded
	// once, one phantom pass, one count and one emit pass over all positions).  A font id of several files (two records merged
	// into one id), a group of one and a family past the budget stay on the single path.  Same families, same output
	void set_family_tables_batched(bool on) { family_tables_batched_ = on; }
	// the font ids of the faces that share their bytes with the ONE file of `font_id` (add_font_named_instances: every record's
	// id, in the table's order, an id two records arrive at twice); empty: an unknown id, an id of several files, a file added
	// any other way
	std::vector<std::string> instance_group(const std::string &font_id) const;
	// faces placed from now on (add_font_instance, _normalized, add_font_named_instances and the named-instance scan) that are
	// glyf + gvar without a readable HVAR take their advances from gvar's phantom points (rule G7 of ttf_face.hpp; default off:
	// their hmtx advances stand).  Not retroactive: stores and families are keyed by serials taken at placement.
	void set_gvar_advances(bool on) { gvar_advances_ = on; }
	// the faces placed so far whose advances follow G7
	uint64_t gvar_advance_faces() const { return gvar_advance_faces_; }
	// with set_glyf_tables_on_device: the glyf fonts of a font id's files built in one call (Renderer::fonts_from_tables)
	void set_glyf_tables_batched(bool on) { glyf_tables_batched_ = on; }
	// uploads every face of the manager that has a resident form now (through lane 0 of every device lane of the renderer);
	// returns the bytes put on the devices
	uint64_t preload_resident_fonts(const Renderer &renderer) const;
	// a renderer with several device lanes: -1 (default) = whole (font, block) tasks per lane unless there are fewer than four
	// non-empty blocks per lane, 0 = always glyph-level shards of every font (+ merge), 1 = always whole tasks.  Same bytes.
	void set_lane_form(int form) { lane_form_ = form; }
	// every glyph of a font id in the form the device's glyf decoder takes (glyf fonts only; tests, inspection)
	bool record_glyf_parts(const std::string &font_id, GlyfPartsBatch &out, std::string *err) const;
	// resident-font form: what a submission of every glyph of the font names, and the description of one of its files
	// (nullptr: unknown font / file, or a face without a resident form)
	bool record_resident(const std::string &font_id, ResidentBatch &out, std::string *err) const { return record_named(font_id, out, false, err); }
	const ResidentTable *resident_table(const std::string &font_id, size_t file_index, std::string *err) const;
	// the same against command fonts (vgsdf_font_create_commands), for every face the reader can read, `glyf` or not
	// (nullptr / false: unknown font / file, or a face whose commands pass what 32-bit offsets address)
	bool record_resident_commands(const std::string &font_id, ResidentBatch &out, std::string *err) const { return record_named(font_id, out, true, err); }
	const CommandTable *command_table(const std::string &font_id, size_t file_index, std::string *err) const;
	// The host half of a resident family (vgsdf_family_create): for every code point the font id maps, up to 0xFFFF and
	// ascending, the file that draws it (first provider wins), its glyph id there, advance, scale and shift_x — the arithmetic
	// of Renderer::record_resident, so the arrays equal those of record_resident / record_resident_commands element for
	// element.  Needs no outline table of either kind.  Built on first use and kept until a file is added to the font id;
	// the pointer stays valid until then (nullptr: unknown font id, or more than 65536 files)
	struct FamilyTable {
		uint64_t serial = 0; // of this build of the table (a rebuilt table is another family on the device)
		size_t n_files = 0;
		// a table the DEVICE builds (family_shell): code_point and advance are the family's read-back, filled when the first
		// device has built it, the other arrays stay empty; refused: the faces' description refuses, the host builds the table
		bool filled = false, refused = false;
		uint32_t plane = 0; // code_point holds the low halves of (plane << 16) | x
		// the plane-0 shell of a font id also keeps its census (vgsdf_family_tables_census, one call per font id): bit p of
		// census_planes says that some block of plane p is listed; census_done 2: the call failed, the block table alone decides
		int census_done = 0;
		uint32_t census_planes = 0;
		std::vector<uint16_t> code_point, font_of, glyph_id;
		std::vector<uint32_t> advance;
		std::vector<double> scale, shift_x;
	};
	const FamilyTable *family_table(const std::string &font_id, std::string *err, uint32_t plane = 0) const;

private:
	using FontEntry = std::map<std::string, FontWrapper>::value_type;
	// the font of an id (nullptr, and "unknown font id ..." in *err: there is none)
	const FontEntry *find_font(const std::string &font_id, std::string *err) const;
	bool record_named(const std::string &font_id, ResidentBatch &out, bool commands, std::string *err) const;
	template <class Table>
	const Table *file_table(const std::string &font_id, size_t file_index, const Table &(Face::*table)() const, const char *why, std::string *err) const;
	using FamilyKey = std::pair<std::string, uint32_t>; // (font id, plane)
	mutable std::map<FamilyKey, std::unique_ptr<FamilyTable>> family_tables_; // the host's tables
	mutable std::map<FamilyKey, std::unique_ptr<FamilyTable>> family_shells_; // set_family_tables_on_device
	// the font id's table as the device builds it: serial and n_files at once, the names once a device has built it (rebuilt, as
	// family_table, when a file is added)
	FamilyTable *family_shell(const std::string &font_id, size_t n_files, uint32_t plane = 0) const;
	mutable std::mutex family_mu_;
	std::mutex &family_mu_of() const { return parent_ ? parent_->family_mu_ : family_mu_; }
	struct Todo {
		const std::string *name;
		const GlyphBlock &block; // lives in its FontWrapper's table
	};
	// One unit of host work: a 64-code-point slice of a task's block, tessellated into the
	// worker's local batch; the ranges say where.
	struct alignas(64) Slice {
		uint32_t task = 0, ci0 = 0, ci1 = 0;
		unsigned worker = 0;
		uint32_t job0 = 0, job1 = 0;       // jobs [job0, job1) of the worker-local batch
		uint32_t raster0 = 0, raster1 = 0; // rasterised glyphs [raster0, raster1) of it
		uint32_t g_raster = 0;             // first raster index in the packed batch
		uint64_t g_seg = 0, g_out = 0;     // first segment / output byte in the packed batch
	};
	struct OSlice { // device front-end: a slice's glyph entries in its worker's OutlineBatch
		uint32_t task = 0;
		unsigned worker = 0;
		uint32_t job0 = 0, job1 = 0;
		uint32_t g_job = 0; // first glyph index in the merged batch
		// commands / command slots, coordinates / parts and bytes: first what the slice added to its worker's batch, noted by the
		// worker while that batch is hot in its cache; the merge's serial pass (which touches no other array) turns the counts
		// into where the first of each lies in the merged batch
		uint32_t g_cmd = 0, g_dat = 0, g_byte = 0;
	};
	struct alignas(128) Worker { // own cache lines: the vector headers inside are written per glyph
		TessScratch scratch;
		GlyphBatch local;
		PackedOutlineBatch olocal;
		GlyfPartsBatch plocal;
		ResidentBatch rlocal;
		char pad[128];
	};
	// One process, N devices (renderer.n_devices() > 1): the glyphs of every font are dealt to the device lanes by
	// estimated cost (shard_glyphs), lane i renders its shard on its own host thread with its own pool, buffers and
	// device contexts, the partial PBFs of a block land side by side in this process's memory and are merged
	// (merge_pbf_partials) — no exchange step; the run counters are summed over the lanes by vgsdf_reduce_counters.
	void render_glyphs_multi(Writer &writer, const Renderer &renderer);
	// a lane of render_glyphs_multi: shares the parent's fonts, renders the glyphs rank `rank` of `world` owns
	FontManager(const FontManager *parent, uint32_t rank, uint32_t world);
	const FontManager *parent_ = nullptr;
public:
	struct CaptureFile { // a file a lane has produced: [at, at + len) of its capture store
		size_t at = 0, len = 0;
	};

private:
	std::vector<uint8_t> capture_store_;     // (a lane's files of the current run: render_glyphs_multi / render_tasks_multi)
	std::vector<CaptureFile> capture_files_;
	std::vector<std::unique_ptr<FontManager>> children_; // lanes, kept between runs (their buffers are grow-only)
	// render_tasks_multi: which lane takes which (font, block) task; kept until a font is added (invalidate_shards)
	struct LanePlan {
		uint32_t world = 0;
		int form = -1;                             // 1: whole tasks only, 2: hybrid (the heaviest blocks split between lanes)
		std::vector<Todo> all;                     // the (font, block) tasks in output order
		std::vector<const std::string *> names;
		static constexpr uint32_t kSplit = 0xFFFFFFFFu;
		std::vector<uint32_t> owner, slot;         // whole task i: its lane and its position among the lane's files;
		                                           // split task: owner = kSplit, slot = index into `splits`
		struct Split {
			uint32_t task, first_part, n_parts;    // parts [first_part, first_part + n_parts) of part_owner / part_slot / part_blocks
		};
		std::vector<Split> splits;
		std::vector<uint32_t> part_owner, part_slot;
		std::deque<GlyphBlock> part_blocks;        // the parts' glyph subsets (a Todo refers to its block)
		std::vector<std::vector<Todo>> lane_tasks;
		std::vector<uint32_t> lane_blocks;         // blocks credited to a lane's counters: its whole tasks + the first parts it holds
		bool accurate = false;                     // weights are the estimated w*h*N per glyph (else: outline sizes)
		double est_max_over_mean = 1.0;            // of the lanes' summed weights
	};
	void build_lane_plan(uint32_t world, int form);
public:
	// Which lane renders which code point of `font_id` on `world` lanes (owner[65536], 0xFF = unmapped) under the plan
	// render_glyphs would use with the present lane form, and how many of the font's blocks are split between lanes.
	// Needs no device: the plan is host arithmetic over the fonts' outlines.
	bool plan_lanes(const std::string &font_id, uint32_t world, std::vector<uint8_t> &owner, uint32_t &n_split_blocks, double *est_max_over_mean, std::string *err);
private:
	LanePlan lane_plan_;
	// shard tables, built once per (font, world, number of files) — on the pool — and shared with the lanes
	struct ShardEntry {
		uint32_t world = 0;
		size_t n_files = 0;
		GlyphShard shard;
	};
	mutable std::map<std::string, ShardEntry> shard_cache_;
	mutable std::mutex shard_mu_;
	const GlyphShard &cached_shard(const std::string &font_id, const FontWrapper &font, uint32_t world) const;
	void invalidate_shards();
	uint64_t reduced_[3] = {0, 0, 0};
	void run_tasks(std::vector<Todo> &tasks, Writer &writer, const Renderer &renderer);
	void render_tasks_multi(Writer &writer, const Renderer &renderer, int form); // N device lanes: whole (font, block) tasks, the heaviest split (form 2)
	void run_tasks_device_front_end(std::vector<Todo> &tasks, Writer &writer, const Renderer &renderer);
	// tessellate tasks [t0, t1) on the pool and pack them (task order, ascending id) into `out`
	void tessellate_and_pack(const std::vector<Todo> &tasks, size_t t0, size_t t1, std::vector<Slice> &slices,
	                         PackedBatch &out);
	ThreadPool &pool();
	unsigned worker_count() const;
	// the block table tasks are built from: the font's own, or its copy filtered to this rank's glyphs
	const std::vector<GlyphBlock> &task_blocks(const std::string &font_id, const FontWrapper &font) const;
	uint32_t shard_rank_ = 0, shard_world_ = 1;
	mutable std::map<std::string, std::vector<GlyphBlock>> shard_blocks_; // per font id, for (shard_rank_, shard_world_)
	std::unique_ptr<ThreadPool> pool_;
	std::vector<Worker> workers_;
	PackedBatch packed_;
	// The form a group of the device front-end is submitted in: the host reader's commands in the packed upload form; the glyphs'
	// `glyf` parts; the glyphs named by (font, glyph id) against the renderer's resident glyf stores / command stores; code-point
	// ranges of the font ids' families over either kind of store
	// ... or over both kinds, store by store (set_mixed_stores)
	enum class GroupForm : uint8_t { Packed, GlyfParts, NamedGlyf, NamedCommands, RangesGlyf, RangesCommands, NamedMixed, RangesMixed };
	// the kind of store a form names its glyphs against: one kind for every file, or per file whichever the file gets
	enum class StoreKind : uint8_t { Glyf, Commands, Mixed };
	// device front-end: the buffers of one group of tasks (<= batch_blocks_ blocks, normally one font)
	struct FeGroup {
		size_t g0 = 0, g1 = 0;
		std::vector<OSlice> slices;
		std::vector<uint32_t> slice_ci;
		MergedOutlines m;
		std::vector<vgsdf_rect> rects;
		std::vector<uint64_t> pbf_at;       // in-place assembly: position of every job's bitmap in `out`
		std::vector<uint32_t> task_g0;      // first job of every task of the group (+ one past the last)
		bool in_place = false;
		struct Piece { // a finished block file: inside `out` (assembled in place) or inside `small`
			const uint8_t *p = nullptr;
			size_t n = 0;
		};
		std::vector<Piece> piece;
		std::vector<uint8_t> small; // blocks without a glyph of the group: name + range only
		std::vector<uint32_t> busy; // the other blocks (indices into the group's tasks): assembled around their bitmaps
		uint64_t n_raster = 0, n_pixels = 0;
		HostBuffer<uint8_t> out{true};
		uint64_t out_bytes = 0, n_segs = 0;
		uint32_t n_jobs = 0;
		GroupForm form = GroupForm::Packed; // what fe_record made of the group
		uint32_t mixed_glyf_stores = 0, mixed_command_stores = 0; // a mixed form: the stores of either kind the group names
		// a group submitted as code-point ranges of resident families (fe_record_ranges): range r is a task of the submission
		bool by_ranges() const { return form == GroupForm::RangesGlyf || form == GroupForm::RangesCommands || form == GroupForm::RangesMixed; }
		struct Ranges {
			std::vector<const vgsdf_family *> families; // of the group's font ids, in task order
			std::vector<const FamilyTable *> tables;    // ... and their host halves
			std::vector<uint16_t> family_of, first, last;
			std::vector<uint32_t> pre;         // bytes in front of the range's first entry: the block header's room, 0 for a block's later runs
			std::vector<uint32_t> entry_first; // the range's first entry in its family's table
			std::vector<uint32_t> task_r0;     // first range of every task of the group (+ one past the last)
			std::vector<uint64_t> extents;     // vgsdf_outlines_task_extents: [ranges + 1]
			void clear()
			{
				families.clear(), tables.clear(), family_of.clear(), first.clear(), last.clear(), pre.clear(), entry_first.clear(), task_r0.clear();
			}
			vgsdf_outlines_ranges view(bool with_pre) const
			{
				return vgsdf_outlines_ranges{(uint32_t)first.size(), (uint32_t)families.size(), families.data(), family_of.data(), first.data(),
				                             last.data(), with_pre ? pre.data() : nullptr};
			}
		} ranges;
	};
	FeGroup fe_group_[2]; // two groups in flight: one on the GPU, one being recorded / encoded
	// Records the group in the first form, of those the switches and the group's faces allow, that takes it (G.form).  renderer /
	// lane: whose device copies of the fonts a group names (nullptr: no such form for this call); allow_glyf is false where a
	// group the device has refused is recorded again: that fallback is the reader's, as ever
	void fe_record(const std::vector<Todo> &tasks, FeGroup &G, bool allow_glyf = true, const Renderer *renderer = nullptr, int lane = 0);
	struct FormList { // the forms to try, in order
		GroupForm form[8];
		unsigned n = 0;
	};
	FormList fe_candidates(bool device_forms, bool glyf_forms, bool by_name, bool by_ranges) const;
	// the one recorder of the forms that merge what the workers record slice by slice, and what differs between them
	// (front_end_dispatch.cpp)
	struct PackedForm;
	struct GlyfForm;
	struct NamedForm;
	template <class Form> bool fe_record_slices(const std::vector<Todo> &tasks, FeGroup &G, Form form, double t0);
	void fe_record_packed(const std::vector<Todo> &tasks, FeGroup &G);
	bool fe_record_glyf(const std::vector<Todo> &tasks, FeGroup &G); // false: not a batch for the device's decoder (fan-out past 32-bit offsets)
	// false: a face of the group has no store of the kind or does not fit the renderer's budget
	// commands: against the faces' command stores (every readable face has one) instead of their glyf stores
	// Mixed: per file the store it gets (file_store); false also when no file of the group gets a glyf store
	bool fe_record_named(const std::vector<Todo> &tasks, FeGroup &G, const Renderer &renderer, int lane, StoreKind kind);
	// false: as above, or a family over the budget.  A supplementary block names the font id's family of ITS plane (device_family);
	// its tasks carry the low halves
	bool fe_record_ranges(const std::vector<Todo> &tasks, FeGroup &G, const Renderer &renderer, int lane, StoreKind kind);
	// the device family of a font id over its files' stores of one kind (nullptr: a file without such a store, or the budget), or
	// (Mixed) over the store each file gets, a family of the mixed kind; *glyf_stores / *command_stores (may be NULL): += the stores of
	// either kind among them
	const vgsdf_family *device_family(const Renderer &renderer, int lane, const std::string &font_id, const FontWrapper &font, StoreKind kind,
	                                  const FamilyTable **table, RenderTimings &counts, uint32_t *glyf_stores = nullptr,
	                                  uint32_t *command_stores = nullptr, uint32_t plane = 0) const;
	// Mixed stores: the store a FILE gets — its glyf store where the face has `glyf` outlines, its font id has not been refused by
	// the decoder and the store can be made (host table or device builder); a command store otherwise.  *glyf says which
	const vgsdf_font *file_store(const Renderer &renderer, int lane, const std::string &font_id, const Face &face, RenderTimings &counts,
	                             bool *glyf) const;
	// whether a mixed form can be worth trying for the fonts of tasks [g0, g1): a `glyf` file of a font id not refused among them
	bool may_mix(const std::vector<Todo> &tasks, size_t g0, size_t g1) const;
	void fe_assemble_ranges(const std::vector<Todo> &tasks, FeGroup &G);
	// fonts (by id) one of whose groups the device's glyf decoder refused (VGSDF_E_GLYF) or whose parts passed the batch bounds:
	// later groups and runs record them with the host's reader at once instead of paying the double path again; cleared
	// with the shard tables when a font is added
	std::set<const std::string *> glyf_refused_;
	void fe_make_slices(const std::vector<Todo> &tasks, FeGroup &G, uint32_t per_slice);
	void fe_layout_common(const std::vector<Todo> &tasks, FeGroup &G); // task_g0, pbf_pre of the merged batch
	void fe_encode_write(const std::vector<Todo> &tasks, FeGroup &G, Writer &writer);
	void fe_prepare_pieces(const std::vector<Todo> &tasks, FeGroup &G);
	void fe_assemble(const std::vector<Todo> &tasks, FeGroup &G);
	void fe_write_pieces(const std::vector<Todo> &tasks, FeGroup &G, Writer &writer);
	static bool glyf_on_device_default()
	{
		const char *e = std::getenv("VG_GLYF_ON_DEVICE");
		return !(e && e[0] == '0');
	}
	bool in_place_pbf_ = true;
	int lane_form_ = -1;
	bool glyf_on_device_ = glyf_on_device_default(); // glyf fonts: the device decodes the glyphs' arrays (VG_GLYF_ON_DEVICE=0 / set_glyf_on_device(false): the host does)
	bool resident_fonts_ = false;
	int resident_commands_ = 0;
	bool mixed_stores_ = false;
	int charstrings_on_device_ = 0;
	bool family_tables_on_device_ = false;
	bool glyf_tables_on_device_ = false;
	bool gvar_on_device_ = false;
	bool glyf_tables_batched_ = false;
	bool gvar_batched_ = false, scan_named_instances_ = false, charstrings_batched_ = false;
	bool gvar_advances_ = false;
	uint64_t gvar_advance_faces_ = 0;
	// the placed faces that share their bytes — the faces add_font_named_instances made of one file, glyf + gvar or CFF2 —, by the
	// address of those bytes, each with the font id it went to (a child manager reads its parent's); a group of one makes no
	// batched call
	struct InstanceGroup {
		std::vector<const Face *> faces;
		std::vector<std::string> ids;
		// charstring2_group(): the faces' CFF2 factors one behind the other, made once (empty with `alike` false: not describable)
		mutable std::once_flag charstring2_once;
		mutable std::vector<float> charstring2_factors;
		mutable bool charstring2_alike = false;
	};
	std::map<const uint8_t *, InstanceGroup> instance_groups_;
	std::map<const Face *, const uint8_t *> instance_bytes_of_; // a grouped face -> its group's key
	const InstanceGroup *instance_group_of(const Face &face) const;
	bool family_tables_batched_ = false;
	// family_tables_batched_: the families of the single-file font ids of `font`'s instance group that the device has yet to
	// build, in one call; the family_from_tables of each behind it finds its family (or goes the way of one that was refused or
	// did not fit); counts into `counts`
	void families_batched(const Renderer &renderer, int lane, const FontWrapper &font, StoreKind kind, RenderTimings &counts) const;
	// gvar_batched_: the command stores of `face`'s group that the device has yet to build, in one call; the gvar_font of each face
	// behind it finds its store (or goes the way of a face that was refused or did not fit); counts into `counts`
	void gvar_stores_batched(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const;
	// charstrings_batched_ (with charstrings_on_device_ 2): the same for the CFF2 faces of `face`'s group; the charstring_font of
	// each face behind it finds its store (or goes the way of one that was refused or did not fit); counts into `counts`
	void charstring2_stores_batched(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const;
	// glyf_tables_batched_: the glyf fonts of `font`'s files that the device has yet to build, in one call; the glyf_store of each
	// file behind it finds its font (or goes the way of a face that was refused or did not fit); counts into `counts`
	void glyf_stores_batched(const Renderer &renderer, int lane, const FontWrapper &font, RenderTimings &counts) const;
	// a face's glyf-kind font on the renderer's device, by either path; counts into `counts`
	const vgsdf_font *glyf_store(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const;
	mutable RenderTimings preload_counts_;
	// a face's command store on the renderer's device, by either path; counts into `counts`
	const vgsdf_font *command_store(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const;
	bool resident_families_ = false;
	bool supplementary_planes_ = false;
	FontWrapper &font_slot(const std::string &font_id); // fonts_[font_id], made with the manager's supplementary switch
	bool device_front_end_ = true; // HIP renderer: flatten on the GPU unless switched off
	bool union_outlines_ = false;
	uint64_t union_stats_[4] = {0, 0, 0, 0};
	struct UnionRun; // (font_manager.cpp)
	std::map<std::string, FontWrapper> fonts_; // reference: HashMap (arbitrary order); sorted here
	bool parallel_;
	unsigned threads_ = 0;       // 0 = hardware_concurrency
	unsigned batch_blocks_ = 256; // blocks per GPU submission (256 = one whole font)
	bool batch_blocks_set_ = false; // false: the device front-end groups by glyph count instead (kFeGlyphBudget)
	RenderTimings timings_;
};

std::string name_to_id(const std::string &name); // manager.rs:141-147

// Combines partial PBFs of ONE block (same font name and range; each holds a disjoint subset of the block's
// glyphs, e.g. one per rank of a glyph-level shard) into the block's PBF: glyph messages are taken as they
// are and written in ascending id, so the result equals the PBF a single process encodes.  Throws
// std::runtime_error on malformed input or when names / ranges differ.
std::vector<uint8_t> merge_pbf_partials(const std::vector<std::pair<const uint8_t *, size_t>> &parts);
// the same for parts that hold consecutive runs of the block's code points, in order: header + the parts' entries as they are
std::vector<uint8_t> concat_pbf_partials(const std::vector<std::pair<const uint8_t *, size_t>> &parts);
// the same without the copy: `head` receives the file's own bytes (length prefix, name and range), `pieces` head + the parts'
// entry regions where they lie — for Writer::write_gather.  false: the parts are not in that form (use merge_pbf_partials)
bool plan_pbf_concat(const std::vector<std::pair<const uint8_t *, size_t>> &parts, std::vector<uint8_t> &head,
                     std::vector<std::pair<const uint8_t *, size_t>> &pieces);

} // namespace vg
