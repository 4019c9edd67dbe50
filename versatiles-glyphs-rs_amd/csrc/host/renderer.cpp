#include "renderer.hpp"

#include <cmath>
#include <cstring>
#include <stdexcept>

namespace vg {

namespace {

// Rust `as i32` / `as u32` on f64: truncate, saturate, NaN -> 0
inline int32_t to_i32(double v)
{
	if (std::isnan(v))
		return 0;
	if (v >= 2147483647.0)
		return INT32_MAX;
	if (v <= -2147483648.0)
		return INT32_MIN;
	return (int32_t)v;
}
inline uint32_t to_u32(double v)
{
	if (std::isnan(v) || v <= 0.0)
		return 0;
	if (v >= 4294967295.0)
		return UINT32_MAX;
	return (uint32_t)v;
}

// a face's loca and glyf as the device's constructors take them
vgsdf_font_tables_desc tables_desc(const FontTables &t)
{
	vgsdf_font_tables_desc d;
	d.num_glyphs = t.num_glyphs, d.loca_entries = t.loca_entries, d.loca_long = t.loca_long;
	d.n_loca_bytes = t.n_loca_bytes, d.n_glyf_bytes = t.n_glyf_bytes;
	d.loca = t.loca, d.glyf = t.glyf;
	return d;
}

} // namespace

void GlyphBatch::clear()
{
	jobs.clear();
	raster_job.clear();
	seg_off.assign(1, 0);
	sx.clear();
	sy.clear();
	ex.clear();
	ey.clear();
	x0.clear();
	y0.clear();
	w.clear();
	h.clear();
	out_off.assign(1, 0);
}

vgsdf_batch GlyphBatch::view() const
{
	vgsdf_batch b;
	b.n_glyphs = (uint32_t)w.size();
	b.seg_off = seg_off.data();
	b.seg_sx = sx.data();
	b.seg_sy = sy.data();
	b.seg_ex = ex.data();
	b.seg_ey = ey.data();
	b.x0 = x0.data();
	b.y0 = y0.data();
	b.w = w.data();
	b.h = h.data();
	b.out_off = out_off.data();
	return b;
}

void GlyphBatch::append(const GlyphBatch &o)
{
	const uint32_t job_base = (uint32_t)jobs.size();
	const uint32_t seg_base = seg_off.back();
	const uint64_t out_base = out_off.back();
	jobs.insert(jobs.end(), o.jobs.begin(), o.jobs.end());
	for (uint32_t j : o.raster_job)
		raster_job.push_back(job_base + j);
	for (size_t i = 1; i < o.seg_off.size(); i++)
		seg_off.push_back(seg_base + o.seg_off[i]);
	sx.insert(sx.end(), o.sx.begin(), o.sx.end());
	sy.insert(sy.end(), o.sy.begin(), o.sy.end());
	ex.insert(ex.end(), o.ex.begin(), o.ex.end());
	ey.insert(ey.end(), o.ey.begin(), o.ey.end());
	x0.insert(x0.end(), o.x0.begin(), o.x0.end());
	y0.insert(y0.end(), o.y0.begin(), o.y0.end());
	w.insert(w.end(), o.w.begin(), o.w.end());
	h.insert(h.end(), o.h.begin(), o.h.end());
	for (size_t i = 1; i < o.out_off.size(); i++)
		out_off.push_back(out_base + o.out_off[i]);
}

void PackedBatch::reserve(uint32_t rasters, uint64_t segs, uint64_t pixels)
{
	seg_off.ensure((size_t)rasters + 1);
	out_off.ensure((size_t)rasters + 1);
	x0.ensure(rasters);
	y0.ensure(rasters);
	w.ensure(rasters);
	h.ensure(rasters);
	sx.ensure(segs);
	sy.ensure(segs);
	ex.ensure(segs);
	ey.ensure(segs);
	out.ensure(pixels);
	seg_off[0] = 0;
	out_off[0] = 0;
}

vgsdf_batch PackedBatch::view() const
{
	vgsdf_batch b;
	b.n_glyphs = n_raster;
	b.seg_off = seg_off.data();
	b.seg_sx = sx.data();
	b.seg_sy = sy.data();
	b.seg_ex = ex.data();
	b.seg_ey = ey.data();
	b.x0 = x0.data();
	b.y0 = y0.data();
	b.w = w.data();
	b.h = h.data();
	b.out_off = out_off.data();
	return b;
}

std::shared_ptr<Renderer> Renderer::create(bool dummy, int device, std::string *err)
{
	return dummy ? new_dummy() : new_precise(device, err);
}

std::shared_ptr<Renderer> Renderer::new_dummy()
{
	std::shared_ptr<Renderer> r(new Renderer());
	r->mode_ = Mode::Dummy;
	return r;
}

std::shared_ptr<Renderer> Renderer::new_precise(int device, std::string *err)
{
	std::shared_ptr<Renderer> r(new Renderer());
	r->mode_ = Mode::Hip;
	r->device_ = device;
	const int rc = vgsdf_create(device, &r->ctx_);
	if (rc != VGSDF_OK) {
		if (err)
			*err = vgsdf_last_error(nullptr);
		return nullptr; // no CPU fallback: the caller must fail
	}
	return r;
}

std::shared_ptr<Renderer> Renderer::new_multi(const std::vector<int> &devices, std::string *err)
{
	if (devices.empty() || devices.size() > 254) {
		if (err)
			*err = "Renderer::new_multi: 1 .. 254 devices";
		return nullptr;
	}
	std::shared_ptr<Renderer> r = new_precise(devices[0], err);
	if (!r)
		return nullptr;
	for (size_t i = 1; i < devices.size(); i++) {
		std::shared_ptr<Renderer> p = new_precise(devices[i], err);
		if (!p)
			return nullptr;
		p->resident_ = r->resident_; // lanes that share a device share the device copies of the fonts
		p->owns_resident_ = false;
		r->peers_.push_back(std::move(p));
	}
	return r;
}

void Renderer::add_counters(uint64_t blocks, uint64_t glyphs, uint64_t pixels) const
{
	if (mode_ != Mode::Hip)
		return;
	std::lock_guard<std::mutex> lock(mu_);
	vgsdf_add_counters(ctx_, blocks, glyphs, pixels);
}

void Renderer::reset_counters() const
{
	for (size_t i = 0; i < n_devices(); i++) {
		const Renderer &l = device_lane(i);
		if (l.mode_ == Mode::Hip) {
			std::lock_guard<std::mutex> lock(l.mu_);
			vgsdf_reset_counters(l.ctx_);
		}
	}
}

void Renderer::reduce_counters(uint64_t out[3]) const
{
	if (mode_ != Mode::Hip)
		throw std::runtime_error("reduce_counters needs the HIP renderer");
	std::vector<vgsdf_ctx *> ctxs;
	for (size_t i = 0; i < n_devices(); i++)
		ctxs.push_back(device_lane(i).ctx_);
	if (vgsdf_reduce_counters(ctxs.data(), (int)ctxs.size(), out) != VGSDF_OK)
		throw std::runtime_error(std::string("vgsdf_reduce_counters: ") + vgsdf_last_error(ctx_));
}

std::string Renderer::reduce_path() const
{
	if (mode_ != Mode::Hip)
		return "";
	return vgsdf_reduce_path(device_lane(0).ctx_);
}

Renderer::~Renderer()
{
	if (owns_resident_ && ctx_) { // (the peers and their contexts are still there: members go after this body)
		for (auto &kv : resident_->families) // (they name the fonts below)
			for (size_t i = 0; i < n_devices(); i++)
				if (device_lane(i).device_ == std::get<0>(kv.first)) {
					vgsdf_family_free(device_lane(i).ctx_, kv.second);
					break;
				}
		for (auto &kv : resident_->fonts)
			for (size_t i = 0; i < n_devices(); i++)
				if (device_lane(i).device_ == kv.first.first) {
					vgsdf_font_free(device_lane(i).ctx_, kv.second);
					break;
				}
		resident_->clear();
	}
	if (ctx2_)
		vgsdf_destroy(ctx2_);
	if (ctx_)
		vgsdf_destroy(ctx_);
}

bool Renderer::prepare(const Face &face, uint32_t index, TessScratch &scratch, GlyphBatch &batch)
{
	// renderer.rs:104 char::from_u32
	if (index > 0x10FFFF || (index >= 0xD800 && index <= 0xDFFF))
		return false;
	const auto glyph_id = face.glyph_index(index); // :106
	if (!glyph_id)
		return false;
	const double scale = (double)GLYPH_SIZE / (double)face.units_per_em(); // :107

	scratch.builder.reset(); // :109-111
	face.outline_glyph(*glyph_id, scratch.builder);
	Rings &rings = scratch.builder.into_rings();

	const double advance_float = (double)face.glyph_hor_advance(*glyph_id).value_or(0) * scale * 0.95; // :115
	const uint32_t advance = to_u32(std::round(advance_float));                                          // :116

	GlyphJob job;
	job.id = index;
	job.advance = advance;
	if (rings.is_empty()) { // :118-120
		batch.jobs.push_back(job);
		return true;
	}
	rings.scale(scale);                                           // :122
	const double dx = ((double)advance - advance_float) / 2.0;   // :130
	rings.translate(Point{dx, 0.0});                              // :131

	const BBox bbox = rings.get_bbox(); // prepare_glyph :64-91
	if (bbox.is_empty()) {
		batch.jobs.push_back(job);
		return true;
	}
	job.x0 = to_i32(std::floor(bbox.min.x)) - BUFFER;
	job.y0 = to_i32(std::floor(bbox.min.y)) - BUFFER;
	job.x1 = to_i32(std::ceil(bbox.max.x)) + BUFFER;
	job.y1 = to_i32(std::ceil(bbox.max.y)) + BUFFER;
	job.width = (uint32_t)(job.x1 - job.x0);
	job.height = (uint32_t)(job.y1 - job.y0);
	job.has_raster = true;

	// Rings::get_segments (rings.rs:75-81): consecutive point pairs, ring by ring
	const std::vector<Point> &pts = rings.points();
	const std::vector<uint32_t> &st = rings.starts();
	const size_t nseg = rings.segment_count();
	const size_t base = batch.sx.size();
	batch.sx.resize(base + nseg);
	batch.sy.resize(base + nseg);
	batch.ex.resize(base + nseg);
	batch.ey.resize(base + nseg);
	size_t k = base;
	for (size_t r = 0; r + 1 < st.size(); r++)
		for (uint32_t i = st[r]; i + 1 < st[r + 1]; i++, k++) {
			batch.sx[k] = pts[i].x;
			batch.sy[k] = pts[i].y;
			batch.ex[k] = pts[i + 1].x;
			batch.ey[k] = pts[i + 1].y;
		}
	job.n_segments = (uint32_t)nseg;
	batch.raster_job.push_back((uint32_t)batch.jobs.size());
	batch.jobs.push_back(job);
	batch.seg_off.push_back((uint32_t)(base + nseg));
	batch.x0.push_back(job.x0);
	batch.y0.push_back(job.y0);
	batch.w.push_back(job.width);
	batch.h.push_back(job.height);
	batch.out_off.push_back(batch.out_off.back() + (uint64_t)job.width * job.height);
	return true;
}

bool Renderer::record(const Face &face, uint32_t index, OutlineBatch &batch)
{
	if (index > 0x10FFFF || (index >= 0xD800 && index <= 0xDFFF)) // renderer.rs:104
		return false;
	const auto glyph_id = face.glyph_index(index); // :106
	if (!glyph_id)
		return false;
	const double scale = (double)GLYPH_SIZE / (double)face.units_per_em(); // :107
	CommandRecorder rec(batch.cmds);
	face.outline_glyph(*glyph_id, rec); // :109-111, callbacks only
	const double advance_float = (double)face.glyph_hor_advance(*glyph_id).value_or(0) * scale * 0.95; // :115
	const uint32_t advance = to_u32(std::round(advance_float));                                          // :116
	GlyphJob job;
	job.id = index;
	job.advance = advance;
	batch.jobs.push_back(job);
	batch.cmd_off.push_back((uint32_t)batch.cmds.size());
	batch.dat_off.push_back(batch.dat_off.back() + rec.n_floats());
	batch.scale.push_back(scale);
	batch.shift_x.push_back(((double)advance - advance_float) / 2.0); // :130
	return true;
}

bool Renderer::record(const Face &face, uint32_t index, PackedOutlineBatch &batch)
{
	if (index > 0x10FFFF || (index >= 0xD800 && index <= 0xDFFF)) // renderer.rs:104
		return false;
	const auto glyph_id = face.glyph_index(index); // :106
	if (!glyph_id)
		return false;
	const double scale = (double)GLYPH_SIZE / (double)face.units_per_em(); // :107
	face.outline_glyph_packed(*glyph_id, batch.kinds, batch.coords); // :109-111, callbacks only
	const double advance_float = (double)face.glyph_hor_advance(*glyph_id).value_or(0) * scale * 0.95; // :115
	const uint32_t advance = to_u32(std::round(advance_float));                                          // :116
	GlyphJob job;
	job.id = index;
	job.advance = advance;
	batch.jobs.push_back(job);
	batch.cmd_off.push_back((uint32_t)batch.kinds.size());
	batch.dat_off.push_back((uint32_t)batch.coords.size());
	batch.scale.push_back(scale);
	batch.shift_x.push_back(((double)advance - advance_float) / 2.0); // :130
	return true;
}

bool Renderer::record_parts(const Face &face, uint32_t index, GlyfPartsBatch &batch)
{
	static_assert(sizeof(GlyfPart) == sizeof(vgsdf_glyf_part), "the host's part record is the ABI's, field for field");
	if (index > 0x10FFFF || (index >= 0xD800 && index <= 0xDFFF)) // renderer.rs:104
		return false;
	const auto glyph_id = face.glyph_index(index); // :106
	if (!glyph_id)
		return false;
	const double scale = (double)GLYPH_SIZE / (double)face.units_per_em(); // :107
	(void)face.glyph_parts(*glyph_id, batch.parts, batch.bytes, batch.slots, &batch.overflow); // :109-111: the outline, undecoded
	const double advance_float = (double)face.glyph_hor_advance(*glyph_id).value_or(0) * scale * 0.95; // :115
	const uint32_t advance = to_u32(std::round(advance_float));                                          // :116
	GlyphJob job;
	job.id = index;
	job.advance = advance;
	batch.jobs.push_back(job);
	batch.slot_off.push_back(batch.slots);
	batch.part_off.push_back((uint32_t)batch.parts.size());
	batch.scale.push_back(scale);
	batch.shift_x.push_back(((double)advance - advance_float) / 2.0); // :130
	return true;
}

bool Renderer::record_resident(const Face &face, uint16_t file, uint32_t index, ResidentBatch &batch)
{
	if (index > 0x10FFFF || (index >= 0xD800 && index <= 0xDFFF)) // renderer.rs:104
		return false;
	const auto glyph_id = face.glyph_index(index); // :106
	if (!glyph_id)
		return false;
	const double scale = (double)GLYPH_SIZE / (double)face.units_per_em(); // :107
	const double advance_float = (double)face.glyph_hor_advance(*glyph_id).value_or(0) * scale * 0.95; // :115
	const uint32_t advance = to_u32(std::round(advance_float));                                          // :116
	GlyphJob job;
	job.id = index;
	job.advance = advance;
	batch.jobs.push_back(job);
	batch.font_of.push_back(file);
	batch.glyph_id.push_back(*glyph_id); // (:109-111: the outline is on the device already)
	batch.scale.push_back(scale);
	batch.shift_x.push_back(((double)advance - advance_float) / 2.0); // :130
	return true;
}

vgsdf_ctx *Renderer::lane_ctx(int lane) const
{
	if (lane == 0)
		return ctx_;
	std::lock_guard<std::mutex> lock(mu_);
	if (!ctx2_ && vgsdf_create(device_, &ctx2_) != VGSDF_OK)
		throw std::runtime_error(std::string("vgsdf_create (second lane): ") + vgsdf_last_error(nullptr));
	return ctx2_;
}

template <class Batch>
void Renderer::submit_on_lane(int lane, const Batch &v, HostBuffer<uint8_t> &out, int (*submit)(vgsdf_ctx *, const Batch *, uint8_t *, size_t),
                              const char *name, uint64_t *block_bytes) const
{
	if (mode_ != Mode::Hip)
		throw std::runtime_error("render_outlines needs the HIP renderer (the device front-end has no CPU form)");
	lane &= 1;
	vgsdf_ctx *c = lane_ctx(lane);
	lane_mu_[lane].lock();
	// one submission: the raster writes into `out` as it stands (capacity kept from earlier groups; first guess
	// 448 bytes per glyph, the average of the fixture fonts) — a second step in wait only when that was too small
	try {
		if (out.capacity() == 0)
			out.ensure((size_t)v.n_glyphs * 480 + 16384);
		std::lock_guard<std::mutex> lock(mu_);
		const bool u = union_outlines(); // no raster behind the plan: wait_outlines renders the union
		if (submit(c, &v, u ? nullptr : out.data(), u ? 0 : out.capacity()) != VGSDF_OK)
			throw std::runtime_error(std::string(name) + ": " + vgsdf_last_error(c));
		if (block_bytes)
			*block_bytes = vgsdf_outlines_resident_upload_bytes(c);
	} catch (...) {
		lane_mu_[lane].unlock();
		throw;
	}
}

void Renderer::submit_outlines(int lane, const vgsdf_outlines_packed &v, HostBuffer<uint8_t> &out) const
{
	submit_on_lane(lane, v, out, vgsdf_outlines_submit_packed, "vgsdf_outlines_submit_packed");
}

void Renderer::submit_outlines(int lane, const vgsdf_outlines_glyf &v, HostBuffer<uint8_t> &out) const
{
	submit_on_lane(lane, v, out, vgsdf_outlines_submit_glyf, "vgsdf_outlines_submit_glyf");
}

void Renderer::submit_outlines(int lane, const vgsdf_outlines_resident &v, HostBuffer<uint8_t> &out, uint64_t *block_bytes, bool mixed) const
{
	if (mixed)
		submit_on_lane(lane, v, out, vgsdf_outlines_submit_resident_mixed, "vgsdf_outlines_submit_resident_mixed", block_bytes);
	else
		submit_on_lane(lane, v, out, vgsdf_outlines_submit_resident, "vgsdf_outlines_submit_resident", block_bytes);
}

template <class Desc, class Made>
Made *Renderer::create_resident(int lane, int (*create)(vgsdf_ctx *, const Desc *, Made **), const Desc &d, const char *name) const
{
	vgsdf_ctx *c = lane_ctx(lane & 1);
	Made *made = nullptr;
	std::lock_guard<std::mutex> lock(mu_);
	if (create(c, &d, &made) != VGSDF_OK)
		throw std::runtime_error(std::string(name) + ": " + vgsdf_last_error(c));
	return made;
}

const vgsdf_font *Renderer::resident_font(int lane, const ResidentTable &t, uint64_t *uploaded_bytes) const
{
	if (mode_ != Mode::Hip || !t.ok)
		return nullptr;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	const auto key = std::make_pair(device_, t.serial);
	if (auto *found = rf.find(rf.fonts, key))
		return found;
	// (what vgsdf_font_create will allocate, to within its rounding: vgsdf::GlyfStoreLayout's arrays without the padding between them)
	const uint64_t want = sizeof(vgsdf_glyf_part) * (uint64_t)t.leaves.size() + t.bytes.size() + 4 * (uint64_t)t.leaf_off.size();
	if (rf.bytes[device_] + want > rf.budget)
		return nullptr;
	vgsdf_font_desc d;
	d.n_glyph_ids = (uint32_t)t.leaf_off.size() - 1;
	d.n_leaves = (uint32_t)t.leaves.size();
	d.n_bytes = (uint32_t)t.bytes.size();
	d.leaf_off = t.leaf_off.data();
	d.leaves = reinterpret_cast<const vgsdf_glyf_part *>(t.leaves.data());
	d.bytes = t.bytes.data();
	vgsdf_font *f = create_resident(lane, vgsdf_font_create, d, "vgsdf_font_create");
	return rf.keep(rf.fonts, key, f, vgsdf_font_device_bytes(f), uploaded_bytes);
}

template <class Build>
const vgsdf_font *Renderer::device_built_font(int lane, ResidentFonts::DeviceBuilt &kind, uint64_t serial, const char *throws_as, Build build,
                                              uint64_t *uploaded_bytes, bool *refused, bool *over_budget, bool *built) const
{
	const auto say = [](bool *flag) {
		if (flag)
			*flag = true;
		return nullptr;
	};
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	const auto key = std::make_pair(device_, serial);
	if (auto *found = rf.find(rf.fonts, key))
		return found;
	const uint64_t room = rf.room(device_);
	if (const auto known = kind.known(key, room))
		return known == ResidentFonts::DeviceBuilt::kUnfit ? say(over_budget) : nullptr;
	vgsdf_ctx *c = lane_ctx(lane & 1);
	vgsdf_font *f = nullptr;
	{
		// the budget as resident_font and command_font hold it: the store's size is known behind the count pass, and checked there,
		// before anything of the store is allocated
		uint64_t want = 0;
		std::lock_guard<std::mutex> lock(mu_);
		const int rc = build(c, room, &f, &want);
		if (rc == VGSDF_E_GLYF || (rc != VGSDF_OK && !throws_as)) {
			kind.remember_refused(key);
			return say(refused);
		}
		if (rc != VGSDF_OK)
			throw std::runtime_error(std::string(throws_as) + ": " + vgsdf_last_error(c));
		if (!f) { // over the budget as it stands
			kind.remember_unfit(key, want);
			return say(over_budget);
		}
	}
	kind.fitted(key);
	if (built)
		*built = true;
	return rf.keep(rf.fonts, key, f, vgsdf_font_device_bytes(f), uploaded_bytes);
}

template <class Job>
void Renderer::settle_batch(ResidentFonts::DeviceBuilt &kind, vgsdf_ctx *c, bool failed, const std::vector<Job> &faces, const std::vector<size_t> &sent,
                            std::vector<vgsdf_font *> &made, const std::vector<int> &status, const std::vector<uint64_t> &needed,
                            std::vector<TablesOutcome> &outcomes) const
{
	ResidentFonts &rf = *resident_;
	for (size_t i = 0; i < sent.size(); i++) {
		TablesOutcome &o = outcomes[sent[i]];
		const auto key = std::make_pair(device_, faces[sent[i]].serial);
		if (failed || status[i] != VGSDF_OK) { // (refused, whatever the reason: the host's way, once)
			kind.remember_refused(key);
			o.refused = true;
			continue;
		}
		if (made[i] && needed[i] > rf.room(device_)) { // (the registry counts allocations, a quarter more than the stores)
			std::lock_guard<std::mutex> lock(mu_);
			(void)vgsdf_font_free(c, made[i]);
			made[i] = nullptr;
		}
		if (!made[i]) { // over the budget as it stands
			kind.remember_unfit(key, needed[i]);
			o.over_budget = true;
			continue;
		}
		kind.fitted(key);
		o.built = true;
		(void)rf.keep(rf.fonts, key, made[i], vgsdf_font_device_bytes(made[i]), &o.uploaded);
	}
}

const vgsdf_font *Renderer::font_from_tables(int lane, uint64_t serial, const FontTables &t, uint64_t *uploaded_bytes, bool *refused,
                                             bool *over_budget, bool *built) const
{
	if (mode_ != Mode::Hip || !t.ok)
		return nullptr;
	// (throws_as NULL: a refusal or a device error, the host's way)
	return device_built_font(lane, resident_->glyf_tables, serial, nullptr, [&](vgsdf_ctx *c, uint64_t room, vgsdf_font **f, uint64_t *want) {
		const vgsdf_font_tables_desc d = tables_desc(t);
		return vgsdf_font_create_tables_within(c, &d, room, f, want);
	}, uploaded_bytes, refused, over_budget, built);
}

void Renderer::fonts_from_tables(int lane, const std::vector<TablesJob> &faces, std::vector<TablesOutcome> &outcomes, uint64_t *calls,
                                 uint64_t *n_sent) const
{
	outcomes.assign(faces.size(), TablesOutcome{});
	if (mode_ != Mode::Hip)
		return;
	// what one call takes (vgsdf.h): 65536 faces, 2^22 glyph ids
	constexpr size_t kMaxFaces = 65536;
	constexpr uint64_t kMaxGlyphIds = 1ull << 22;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	std::vector<size_t> sent;
	std::vector<vgsdf_font_tables_desc> descs;
	std::vector<vgsdf_font *> made;
	std::vector<int> status;
	std::vector<uint64_t> needed;
	auto flush = [&] {
		if (sent.empty())
			return;
		made.assign(sent.size(), nullptr), status.assign(sent.size(), 0), needed.assign(sent.size(), 0);
		vgsdf_ctx *c = lane_ctx(lane & 1);
		int rc;
		{
			std::lock_guard<std::mutex> lock(mu_);
			rc = vgsdf_fonts_create_tables_within(c, descs.data(), (uint32_t)descs.size(), rf.room(device_), made.data(), status.data(), needed.data());
		}
		*calls += 1, *n_sent += sent.size();
		settle_batch(rf.glyf_tables, c, rc != VGSDF_OK, faces, sent, made, status, needed, outcomes); // (a device error: the host's way)
		sent.clear(), descs.clear();
	};
	uint64_t glyph_ids = 0;
	std::set<uint64_t> seen;
	for (size_t i = 0; i < faces.size(); i++) {
		const FontTables &t = faces[i].tables;
		const auto key = std::make_pair(device_, faces[i].serial);
		if (!t.ok || rf.find(rf.fonts, key) || rf.glyf_tables.known(key, rf.room(device_)))
			continue; // (font_from_tables says over_budget when it is asked)
		if (!seen.insert(faces[i].serial).second)
			continue; // (a face named twice: one font)
		if (sent.size() == kMaxFaces || glyph_ids + t.num_glyphs > kMaxGlyphIds)
			flush(), glyph_ids = 0;
		sent.push_back(i), descs.push_back(tables_desc(t));
		glyph_ids += t.num_glyphs;
	}
	flush();
}

const vgsdf_font *Renderer::command_font(int lane, const CommandTable &t, uint64_t *uploaded_bytes) const
{
	if (mode_ != Mode::Hip || !t.ok)
		return nullptr;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	const auto key = std::make_pair(device_, t.serial);
	if (auto *found = rf.find(rf.fonts, key))
		return found;
	// (what vgsdf_font_create_commands will keep, to within its rounding: records | cmd_off | context bytes)
	static_assert(vgsdf::CommandStoreLayout(0, 1).total - vgsdf::CommandStoreLayout(0, 0).total == CommandTable::kStoreBytesPerCmd, "the reader's command budget (ttf_face.cpp) counts the store's bytes per command");
	const uint64_t want = vgsdf::CommandStoreLayout(t.cmd_off.size() - 1, t.kinds.size()).total;
	if (rf.bytes[device_] + want > rf.budget)
		return nullptr;
	vgsdf_font_cmds_desc d;
	d.n_glyph_ids = (uint32_t)t.cmd_off.size() - 1;
	d.n_cmds = (uint32_t)t.kinds.size();
	d.n_floats = (uint32_t)t.coords.size();
	d.cmd_off = t.cmd_off.data();
	d.dat_off = t.dat_off.data();
	d.kinds = t.kinds.data();
	d.coords = t.coords.data();
	vgsdf_font *f = create_resident(lane, vgsdf_font_create_commands, d, "vgsdf_font_create_commands");
	return rf.keep(rf.fonts, key, f, vgsdf_font_device_bytes(f), uploaded_bytes);
}

const vgsdf_font *Renderer::charstring_font(int lane, const CharstringTable &t, uint64_t *uploaded_bytes, bool *refused, bool *over_budget) const
{
	if (mode_ != Mode::Hip || !t.ok)
		return nullptr;
	vgsdf_font_charstrings2_desc d2{};
	vgsdf_font_charstrings_desc &d = d2.charstrings;
	d2.n_sets = (uint32_t)t.set_ok.size();
	d2.n_factors = (uint32_t)t.factors.size();
	d2.set_ok = t.set_ok.data();
	d2.set_off = t.set_off.data();
	d2.factors = t.factors.data();
	d.n_glyph_ids = (uint32_t)t.cs_off.size() - 1;
	d.n_bytes = (uint32_t)t.bytes.size();
	d.bytes = t.bytes.data();
	d.cs_off = t.cs_off.data();
	d.n_gsubrs = (uint32_t)t.gsubr_off.size() - 1;
	d.gsubr_off = t.gsubr_off.data();
	d.n_fds = t.n_fds;
	d.lsubr_first = t.lsubr_first.data();
	d.lsubr_off = t.lsubr_off.data();
	d.fd_of = t.fd_of.empty() ? nullptr : t.fd_of.data();
	return device_built_font(lane, resident_->charstrings, t.serial, "vgsdf_font_create_charstrings", [&](vgsdf_ctx *c, uint64_t room, vgsdf_font **f, uint64_t *want) {
		return t.cff2 ? vgsdf_font_create_charstrings2_within(c, &d2, room, f, want) : vgsdf_font_create_charstrings_within(c, &d, room, f, want);
	}, uploaded_bytes, refused, over_budget, nullptr);
}

const vgsdf_font *Renderer::gvar_font(int lane, uint64_t serial, const GvarTables &t, uint64_t *uploaded_bytes, bool *refused, bool *over_budget) const
{
	if (mode_ != Mode::Hip || !t.ok)
		return nullptr;
	return device_built_font(lane, resident_->gvar, serial, "vgsdf_font_create_gvar", [&](vgsdf_ctx *c, uint64_t room, vgsdf_font **f, uint64_t *want) {
		vgsdf_font_gvar_desc d{};
		d.tables = tables_desc(t.tables);
		d.gvar = t.gvar, d.gvar_len = t.gvar_len, d.n_axes = t.n_axes, d.coords = t.coords;
		return vgsdf_font_create_gvar_within(c, &d, room, f, want);
	}, uploaded_bytes, refused, over_budget, nullptr);
}

void Renderer::gvar_fonts(int lane, const std::vector<GvarJob> &faces, std::vector<TablesOutcome> &outcomes, uint64_t *calls, uint64_t *n_sent) const
{
	outcomes.assign(faces.size(), TablesOutcome{});
	if (mode_ != Mode::Hip)
		return;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	std::vector<size_t> sent;
	std::vector<int16_t> coords;
	const GvarTables *first = nullptr;
	auto flush = [&] {
		if (sent.empty())
			return;
		const GvarTables &t = *first;
		vgsdf_fonts_gvar_desc d{};
		d.tables = tables_desc(t.tables);
		d.gvar = t.gvar, d.gvar_len = t.gvar_len, d.n_axes = t.n_axes, d.coords = coords.data(), d.n_positions = (uint32_t)sent.size();
		std::vector<vgsdf_font *> made(sent.size(), nullptr);
		std::vector<int> status(sent.size(), 0);
		std::vector<uint64_t> needed(sent.size(), 0);
		vgsdf_ctx *c = lane_ctx(lane & 1);
		int rc;
		{
			std::lock_guard<std::mutex> lock(mu_);
			rc = vgsdf_fonts_create_gvar_within(c, &d, rf.room(device_), made.data(), status.data(), needed.data());
		}
		if (rc != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_fonts_create_gvar: ") + vgsdf_last_error(c));
		*calls += 1, *n_sent += sent.size();
		settle_batch(rf.gvar, c, false, faces, sent, made, status, needed, outcomes); // (refused at this position, or whatever the position)
		sent.clear(), coords.clear();
	};
	std::set<uint64_t> seen;
	for (size_t i = 0; i < faces.size(); i++) {
		const GvarTables &t = faces[i].tables;
		const auto key = std::make_pair(device_, faces[i].serial);
		if (!t.ok || rf.find(rf.fonts, key) || rf.gvar.known(key, rf.room(device_)))
			continue; // (gvar_font says over_budget when it is asked)
		if (!seen.insert(faces[i].serial).second)
			continue; // (a face named twice: one store)
		if (!first)
			first = &t;
		if (t.gvar != first->gvar || t.n_axes != first->n_axes || t.tables.glyf != first->tables.glyf || t.tables.loca != first->tables.loca)
			continue; // (not over the first face's tables: its own gvar_font builds it)
		if (sent.size() == VGSDF_GVAR_MAX_POSITIONS)
			flush();
		sent.push_back(i);
		coords.insert(coords.end(), t.coords, t.coords + t.n_axes);
	}
	flush();
}

void Renderer::charstring2_fonts(int lane, const std::vector<Charstring2Job> &faces, std::vector<TablesOutcome> &outcomes, uint64_t *calls,
                                 uint64_t *n_sent) const
{
	outcomes.assign(faces.size(), TablesOutcome{});
	if (mode_ != Mode::Hip)
		return;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	std::vector<size_t> sent;
	std::vector<float> factors;
	const CharstringTable *first = nullptr;
	auto flush = [&] {
		if (sent.empty())
			return;
		const CharstringTable &t = *first;
		vgsdf_fonts_charstrings2_desc d{};
		vgsdf_font_charstrings_desc &cs = d.face.charstrings;
		cs.n_glyph_ids = (uint32_t)t.cs_off.size() - 1;
		cs.n_bytes = (uint32_t)t.bytes.size();
		cs.bytes = t.bytes.data();
		cs.cs_off = t.cs_off.data();
		cs.n_gsubrs = (uint32_t)t.gsubr_off.size() - 1;
		cs.gsubr_off = t.gsubr_off.data();
		cs.n_fds = t.n_fds;
		cs.lsubr_first = t.lsubr_first.data();
		cs.lsubr_off = t.lsubr_off.data();
		cs.fd_of = nullptr;
		d.face.n_sets = (uint32_t)t.set_ok.size();
		d.face.n_factors = (uint32_t)t.factors.size();
		d.face.set_ok = t.set_ok.data();
		d.face.set_off = t.set_off.data();
		d.face.factors = factors.data();
		d.n_positions = (uint32_t)sent.size();
		std::vector<vgsdf_font *> made(sent.size(), nullptr);
		std::vector<int> status(sent.size(), 0);
		std::vector<uint64_t> needed(sent.size(), 0);
		vgsdf_ctx *c = lane_ctx(lane & 1);
		int rc;
		{
			std::lock_guard<std::mutex> lock(mu_);
			rc = vgsdf_fonts_create_charstrings2_within(c, &d, rf.room(device_), made.data(), status.data(), needed.data());
		}
		if (rc != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_fonts_create_charstrings2: ") + vgsdf_last_error(c));
		*calls += 1, *n_sent += sent.size();
		settle_batch(rf.charstrings, c, false, faces, sent, made, status, needed, outcomes); // (refused at this position)
		sent.clear(), factors.clear();
	};
	std::set<uint64_t> seen;
	for (size_t i = 0; i < faces.size(); i++) {
		const CharstringTable *t = faces[i].table;
		const auto key = std::make_pair(device_, faces[i].serial);
		if (!t || !t->ok || !t->cff2 || rf.find(rf.fonts, key) || rf.charstrings.known(key, rf.room(device_)))
			continue; // (charstring_font says over_budget when it is asked)
		if (!seen.insert(faces[i].serial).second)
			continue; // (a face named twice: one store)
		if (!first)
			first = t;
		if (t != first && !t->same_face(*first))
			continue; // (not the first face's charstrings: its own charstring_font builds it)
		if (sent.size() == VGSDF_CHARSTRING2_MAX_POSITIONS)
			flush();
		sent.push_back(i);
		factors.insert(factors.end(), t->factors.begin(), t->factors.end());
	}
	flush();
}

const vgsdf_family *Renderer::family(int lane, const FamilyArrays &t, const std::vector<const vgsdf_font *> &fonts, int kind,
                                     uint64_t *uploaded_bytes) const
{
	if (mode_ != Mode::Hip)
		return nullptr;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	const auto key = std::make_tuple(device_, t.serial, kind);
	if (auto *found = rf.find(rf.families, key))
		return found;
	const uint64_t want = vgsdf::FamilyTableLayout(t.code_point->size()).bytes;
	if (rf.bytes[device_] + want > rf.budget)
		return nullptr;
	vgsdf_family_desc d;
	d.n_fonts = (uint32_t)fonts.size();
	d.fonts = fonts.data();
	d.n_entries = (uint32_t)t.code_point->size();
	d.code_point = t.code_point->data();
	d.font_of = t.font_of->data();
	d.glyph_id = t.glyph_id->data();
	d.advance = t.advance->data();
	d.scale = t.scale->data();
	d.shift_x = t.shift_x->data();
	// (plane 0 through vgsdf_family_create_at is the family vgsdf_family_create / _mixed makes)
	static thread_local uint32_t at_plane;
	at_plane = t.plane;
	vgsdf_family *f = kind == kFamilyMixed
	                      ? create_resident(lane, +[](vgsdf_ctx *c, const vgsdf_family_desc *in, vgsdf_family **out) { return vgsdf_family_create_at(c, in, VGSDF_FAMILY_MIXED, at_plane, out); }, d, "vgsdf_family_create_at")
	                      : create_resident(lane, +[](vgsdf_ctx *c, const vgsdf_family_desc *in, vgsdf_family **out) { return vgsdf_family_create_at(c, in, VGSDF_FAMILY_ONE_KIND, at_plane, out); }, d, "vgsdf_family_create_at");
	return rf.keep(rf.families, key, f, vgsdf_family_device_bytes(f), uploaded_bytes);
}

const vgsdf_family *Renderer::family_from_tables(int lane, uint64_t serial, const std::vector<vgsdf_face_tables> &tables,
                                                 const std::vector<const vgsdf_font *> &fonts, int kind, uint64_t *uploaded_bytes, int *refused,
                                                 bool *built, const std::vector<vgsdf_face_variation> &variation,
                                                 const std::vector<const vgsdf_font_gvar_desc *> &gvar, uint32_t plane) const
{
	if (mode_ != Mode::Hip)
		return nullptr;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	const auto key = std::make_tuple(device_, serial, kind);
	if (auto *found = rf.find(rf.families, key))
		return found;
	if (plane && (!variation.empty() || !gvar.empty())) { // (the caller's to keep: the _var and _gvar constructors are plane 0)
		*refused = 1;
		return nullptr;
	}
	if (rf.refused_family_tables.count(key)) {
		*refused = 2;
		return nullptr;
	}
	vgsdf_family_tables_desc d;
	d.n_fonts = (uint32_t)fonts.size();
	d.fonts = fonts.data();
	d.tables = tables.data();
	vgsdf_ctx *c = lane_ctx(lane & 1);
	vgsdf_family *f = nullptr;
	{
		std::lock_guard<std::mutex> lock(mu_);
		const vgsdf_face_variation *var = variation.empty() ? nullptr : variation.data();
		if (tables.size() != fonts.size() || (var && variation.size() != fonts.size()) || (!gvar.empty() && gvar.size() != fonts.size()) ||
		    (!gvar.empty() ? (kind == kFamilyMixed ? vgsdf_family_create_tables_gvar_mixed(c, &d, var, gvar.data(), &f)
		                                          : vgsdf_family_create_tables_gvar(c, &d, var, gvar.data(), &f))
		     : var ? (kind == kFamilyMixed ? vgsdf_family_create_tables_var_mixed(c, &d, var, &f) : vgsdf_family_create_tables_var(c, &d, var, &f))
		     : plane ? vgsdf_family_create_tables_at(c, &d, kind == kFamilyMixed ? VGSDF_FAMILY_MIXED : VGSDF_FAMILY_ONE_KIND, plane, &f)
		         : (kind == kFamilyMixed ? vgsdf_family_create_tables_mixed(c, &d, &f) : vgsdf_family_create_tables(c, &d, &f))) != VGSDF_OK) {
			rf.refused_family_tables.insert(key);
			*refused = 1;
			return nullptr;
		}
		// the budget as family() holds it: the table's size is known behind the count pass
		const uint64_t want = vgsdf::FamilyTableLayout(vgsdf_family_count(f, 0, 0xFFFF)).bytes;
		if (rf.bytes[device_] + want > rf.budget) {
			(void)vgsdf_family_free(c, f);
			return nullptr;
		}
	}
	*built = true;
	return rf.keep(rf.families, key, f, vgsdf_family_device_bytes(f), uploaded_bytes);
}

bool Renderer::family_census(int lane, const std::vector<vgsdf_face_tables> &tables, uint32_t *planes) const
{
	if (mode_ != Mode::Hip || tables.empty())
		return false;
	vgsdf_family_tables_desc d;
	d.n_fonts = (uint32_t)tables.size();
	d.fonts = nullptr; // (the census does not look at fonts)
	d.tables = tables.data();
	uint32_t bits[VGSDF_CENSUS_WORDS];
	{
		std::lock_guard<std::mutex> lock(mu_);
		if (vgsdf_family_tables_census(lane_ctx(lane & 1), &d, bits) != VGSDF_OK)
			return false;
	}
	*planes = 0;
	for (uint32_t w = 0; w < VGSDF_CENSUS_WORDS; w++) // 256 blocks, 8 words, to a plane
		if (bits[w])
			*planes |= 1u << (w / 8);
	return true;
}

void Renderer::families_from_tables(int lane, const std::vector<FamilyJob> &jobs, int kind, std::vector<FamilyOutcome> &outcomes, uint64_t *calls,
                                    uint64_t *n_families) const
{
	outcomes.assign(jobs.size(), FamilyOutcome{});
	if (mode_ != Mode::Hip)
		return;
	ResidentFonts &rf = *resident_;
	std::lock_guard<std::mutex> table_lock(rf.mu);
	std::vector<size_t> sent;
	const FamilyJob *first = nullptr;
	auto flush = [&] {
		if (sent.empty())
			return;
		const FamilyTables &t = *first->tables;
		std::vector<const vgsdf_font *> fonts;
		std::vector<vgsdf_face_variation> var;
		std::vector<int16_t> coords;
		for (size_t i : sent) {
			const FamilyTables &ti = *jobs[i].tables;
			fonts.push_back(jobs[i].font);
			if (t.hvar)
				var.push_back(vgsdf_face_variation{ti.hvar, ti.hvar_len, ti.hvar_store, ti.hvar_map, ti.region_scalars.data(), (uint32_t)ti.region_scalars.size()});
			if (first->gvar.ok)
				coords.insert(coords.end(), jobs[i].gvar.coords, jobs[i].gvar.coords + jobs[i].gvar.n_axes);
		}
		vgsdf_fonts_gvar_desc g{};
		if (first->gvar.ok) {
			const GvarTables &gt = first->gvar;
			g.tables = tables_desc(gt.tables);
			g.gvar = gt.gvar, g.gvar_len = gt.gvar_len, g.n_axes = gt.n_axes, g.coords = coords.data(), g.n_positions = (uint32_t)sent.size();
		}
		vgsdf_families_tables_desc d{};
		d.n_positions = (uint32_t)sent.size();
		d.fonts = fonts.data();
		d.tables.cmap = t.cmap, d.tables.cmap_len = t.cmap_len, d.tables.hmtx = t.hmtx, d.tables.hmtx_len = t.hmtx_len;
		d.tables.units_per_em = t.units_per_em, d.tables.num_glyphs = t.num_glyphs, d.tables.num_hmetrics = t.num_hmetrics;
		d.tables.n_subtables = (uint16_t)t.subtable_off.size();
		d.tables.subtable_off = t.subtable_off.data(), d.tables.subtable_format = t.subtable_format.data();
		d.var = var.empty() ? nullptr : var.data();
		d.gvar = first->gvar.ok ? &g : nullptr;
		std::vector<vgsdf_family *> made(sent.size(), nullptr);
		std::vector<int> status(sent.size(), 0);
		vgsdf_ctx *c = lane_ctx(lane & 1);
		std::lock_guard<std::mutex> lock(mu_);
		const int rc = kind == kFamilyMixed ? vgsdf_families_create_tables_mixed(c, &d, made.data(), status.data())
		                                    : vgsdf_families_create_tables(c, &d, made.data(), status.data());
		*calls += 1;
		for (size_t k = 0; k < sent.size(); k++) {
			const auto key = std::make_tuple(device_, jobs[sent[k]].serial, kind);
			FamilyOutcome &o = outcomes[sent[k]];
			if (rc != VGSDF_OK || status[k] != VGSDF_OK) { // (the whole call, or this position alone: the host's way, for good)
				rf.refused_family_tables.insert(key);
				o.refused = true;
				continue;
			}
			// the budget as family() holds it
			const uint64_t want = vgsdf::FamilyTableLayout(vgsdf_family_count(made[k], 0, 0xFFFF)).bytes;
			if (rf.bytes[device_] + want > rf.budget) {
				(void)vgsdf_family_free(c, made[k]);
				continue;
			}
			o.built = true;
			*n_families += 1;
			rf.keep(rf.families, key, made[k], vgsdf_family_device_bytes(made[k]), &o.uploaded);
		}
		sent.clear();
	};
	std::set<uint64_t> seen;
	for (size_t i = 0; i < jobs.size(); i++) {
		const FamilyJob &j = jobs[i];
		const auto key = std::make_tuple(device_, j.serial, kind);
		if (!j.tables || !j.tables->ok || !j.font || rf.find(rf.families, key) || rf.refused_family_tables.count(key))
			continue;
		if (!seen.insert(j.serial).second)
			continue; // (a family named twice: one family)
		if (!first)
			first = &j;
		const FamilyTables &a = *j.tables, &b = *first->tables;
		if (a.cmap != b.cmap || a.hmtx != b.hmtx || a.hvar != b.hvar || a.hvar_len != b.hvar_len || a.hvar_store != b.hvar_store ||
		    a.hvar_map != b.hvar_map || a.region_scalars.size() != b.region_scalars.size() || j.gvar.ok != first->gvar.ok ||
		    (j.gvar.ok && (j.gvar.gvar != first->gvar.gvar || j.gvar.n_axes != first->gvar.n_axes || j.gvar.tables.glyf != first->gvar.tables.glyf ||
		                   j.gvar.tables.loca != first->gvar.tables.loca)))
			continue; // (not over the first job's tables: its own family_from_tables builds it)
		if (sent.size() == VGSDF_FAMILY_MAX_POSITIONS)
			flush();
		sent.push_back(i);
	}
	flush();
}

void Renderer::family_names(int lane, const vgsdf_family *family, std::vector<uint16_t> &code_point, std::vector<uint32_t> &advance) const
{
	vgsdf_ctx *c = lane_ctx(lane & 1);
	const uint32_t n = vgsdf_family_count(family, 0, 0xFFFF);
	code_point.assign(n, 0);
	advance.assign(n, 0);
	std::lock_guard<std::mutex> lock(mu_);
	if (vgsdf_family_read(c, family, nullptr, code_point.data(), nullptr, nullptr, advance.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != VGSDF_OK)
		throw std::runtime_error(std::string("vgsdf_family_read: ") + vgsdf_last_error(c));
}

void Renderer::submit_ranges(int lane, const vgsdf_outlines_ranges &v, uint32_t n_glyphs, HostBuffer<uint8_t> &out, uint64_t *block_bytes) const
{
	if (mode_ != Mode::Hip)
		throw std::runtime_error("render_outlines needs the HIP renderer (the device front-end has no CPU form)");
	lane &= 1;
	vgsdf_ctx *c = lane_ctx(lane);
	lane_mu_[lane].lock();
	try { // (as submit_on_lane)
		if (out.capacity() == 0)
			out.ensure((size_t)n_glyphs * 480 + 16384);
		std::lock_guard<std::mutex> lock(mu_);
		const bool u = union_outlines(); // (as submit_on_lane)
		if (vgsdf_outlines_submit_ranges(c, &v, u ? nullptr : out.data(), u ? 0 : out.capacity()) != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_outlines_submit_ranges: ") + vgsdf_last_error(c));
		if (block_bytes)
			*block_bytes = vgsdf_outlines_resident_upload_bytes(c);
	} catch (...) {
		lane_mu_[lane].unlock();
		throw;
	}
}

void Renderer::task_extents(int lane, std::vector<uint64_t> &begin, uint32_t n_tasks) const
{
	lane &= 1;
	vgsdf_ctx *c = lane == 0 ? ctx_ : ctx2_;
	begin.assign((size_t)n_tasks + 1, 0);
	std::unique_lock<std::mutex> lock(mu_, std::defer_lock);
	if (lane == 0)
		lock.lock();
	if (vgsdf_outlines_task_extents(c, begin.data()) != VGSDF_OK)
		throw std::runtime_error(std::string("vgsdf_outlines_task_extents: ") + vgsdf_last_error(c));
}

void Renderer::set_resident_budget(uint64_t bytes_per_device)
{
	std::lock_guard<std::mutex> lock(resident_->mu);
	resident_->budget = bytes_per_device;
}

uint64_t Renderer::resident_bytes(int device) const
{
	std::lock_guard<std::mutex> lock(resident_->mu);
	auto it = resident_->bytes.find(device);
	return it == resident_->bytes.end() ? 0 : it->second;
}

bool Renderer::peek_outlines(int lane, std::vector<vgsdf_rect> &rects, uint64_t &out_bytes, uint32_t n_glyphs,
                             std::vector<uint64_t> *pbf_at) const
{
	lane &= 1;
	vgsdf_ctx *c = lane == 0 ? ctx_ : ctx2_;
	rects.assign(n_glyphs, vgsdf_rect{});
	out_bytes = 0;
	int in_place = 0;
	std::unique_lock<std::mutex> lock(mu_, std::defer_lock);
	if (lane == 0)
		lock.lock();
	if (vgsdf_outlines_peek(c, rects.data(), &out_bytes, &in_place) != VGSDF_OK)
		throw std::runtime_error(std::string("vgsdf_outlines_peek: ") + vgsdf_last_error(c));
	if (in_place && pbf_at) {
		pbf_at->assign(n_glyphs, 0);
		if (n_glyphs && vgsdf_outlines_pbf_positions(c, pbf_at->data()) != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_outlines_pbf_positions: ") + vgsdf_last_error(c));
	}
	return in_place != 0;
}

void Renderer::wait_outlines(int lane, std::vector<vgsdf_rect> &rects, HostBuffer<uint8_t> &out, uint64_t &out_bytes,
                             uint64_t &n_segments, uint32_t n_glyphs, std::vector<uint64_t> *pbf_at) const
{
	lane &= 1;
	vgsdf_ctx *c = lane == 0 ? ctx_ : ctx2_;
	out_bytes = n_segments = 0;
	struct Unlock {
		std::mutex &m;
		~Unlock() { m.unlock(); }
	} unlock{lane_mu_[lane]};
	rects.assign(n_glyphs, vgsdf_rect{});
	int rendered = 0;
	// lane 0 shares its context with the one-call entry points (render_batch, ...): keep them out while it is in use
	std::unique_lock<std::mutex> lock(mu_, std::defer_lock);
	if (lane == 0)
		lock.lock();
	if (const int rc = vgsdf_outlines_wait(c, rects.data(), &out_bytes, &n_segments, &rendered); rc != VGSDF_OK) {
		if (rc == VGSDF_E_GLYF)
			throw GlyfEntryError(std::string("vgsdf_outlines_wait: ") + vgsdf_last_error(c));
		throw std::runtime_error(std::string("vgsdf_outlines_wait: ") + vgsdf_last_error(c));
	}
	if (!rendered && out_bytes) {
		if (union_outlines()) {
			std::vector<uint8_t> state(n_glyphs);
			if (vgsdf_outlines_union(c, state.data(), nullptr) != VGSDF_OK)
				throw std::runtime_error(std::string("vgsdf_outlines_union: ") + vgsdf_last_error(c));
			count_union_states(state);
		}
		out.ensure((size_t)out_bytes + 1);
		if (vgsdf_outlines_render(c, out.data()) != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_outlines_render: ") + vgsdf_last_error(c));
	}
	if (pbf_at) { // in-place PBF assembly: where the device placed the bitmaps in the arena `out`
		pbf_at->assign(n_glyphs, 0);
		if (n_glyphs && vgsdf_outlines_pbf_positions(c, pbf_at->data()) != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_outlines_pbf_positions: ") + vgsdf_last_error(c));
	}
}

void Renderer::render_outlines(const vgsdf_outlines &v, std::vector<vgsdf_rect> &rects, HostBuffer<uint8_t> &out,
                               uint64_t &out_bytes, uint64_t &n_segments) const
{
	rects.assign(v.n_glyphs, vgsdf_rect{});
	out_bytes = n_segments = 0;
	if (v.n_glyphs == 0)
		return;
	if (mode_ != Mode::Hip)
		throw std::runtime_error("render_outlines needs the HIP renderer (the device front-end has no CPU form)");
	std::lock_guard<std::mutex> lane(lane_mu_[0]);
	std::lock_guard<std::mutex> lock(mu_);
	if (out.capacity() == 0)
		out.ensure((size_t)v.n_glyphs * 448 + 4096);
	int rendered = 0;
	const bool u = union_outlines();
	if (vgsdf_outlines_render_into(ctx_, &v, rects.data(), u ? nullptr : out.data(), u ? 0 : out.capacity(), &out_bytes, &n_segments, &rendered) != VGSDF_OK)
		throw std::runtime_error(std::string("vgsdf_outlines_render_into: ") + vgsdf_last_error(ctx_));
	if (!rendered && out_bytes) {
		if (u) {
			std::vector<uint8_t> state(v.n_glyphs);
			if (vgsdf_outlines_union(ctx_, state.data(), nullptr) != VGSDF_OK)
				throw std::runtime_error(std::string("vgsdf_outlines_union: ") + vgsdf_last_error(ctx_));
			count_union_states(state);
		}
		out.ensure((size_t)out_bytes + 1);
		if (vgsdf_outlines_render(ctx_, out.data()) != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_outlines_render: ") + vgsdf_last_error(ctx_));
	}
}

void Renderer::set_union_outlines(bool on) const
{
	union_outlines_.store(on);
	for (const auto &p : peers_)
		p->set_union_outlines(on);
}

void Renderer::take_union_stats(uint64_t by_state[4]) const
{
	for (int s = 0; s < 4; s++)
		by_state[s] = union_seen_[s].exchange(0);
	for (const auto &p : peers_) {
		uint64_t theirs[4];
		p->take_union_stats(theirs);
		for (int s = 0; s < 4; s++)
			by_state[s] += theirs[s];
	}
}

void Renderer::count_union_states(const std::vector<uint8_t> &state) const
{
	uint64_t seen[4] = {0, 0, 0, 0};
	for (uint8_t s : state)
		seen[s & 3]++;
	for (int s = 0; s < 4; s++)
		union_seen_[s] += seen[s];
}

void Renderer::render_view(const vgsdf_batch &v, uint8_t *out) const
{
	if (!union_outlines()) {
		if (vgsdf_render_batch(ctx_, &v, out) != VGSDF_OK)
			throw std::runtime_error(std::string("vgsdf_render_batch: ") + vgsdf_last_error(ctx_));
		return;
	}
	vgsdf_dbatch *in = nullptr, *un = nullptr;
	std::vector<uint8_t> state(v.n_glyphs);
	const char *step = "vgsdf_batch_upload";
	int rc = vgsdf_batch_upload(ctx_, &v, &in);
	if (rc == VGSDF_OK)
		step = "vgsdf_batch_union", rc = vgsdf_batch_union(ctx_, in, &un, state.data());
	if (rc == VGSDF_OK)
		step = "vgsdf_batch_launch", rc = vgsdf_batch_launch(ctx_, un);
	if (rc == VGSDF_OK)
		step = "vgsdf_batch_download", rc = vgsdf_batch_download(ctx_, un, out);
	const std::string what = rc == VGSDF_OK ? std::string() : std::string(step) + ": " + vgsdf_last_error(ctx_);
	vgsdf_batch_free(ctx_, un);
	vgsdf_batch_free(ctx_, in);
	if (rc != VGSDF_OK)
		throw std::runtime_error(what);
	count_union_states(state);
}

void Renderer::render_batch(const GlyphBatch &batch, uint8_t *out) const
{
	if (batch.n_raster() == 0)
		return;
	if (mode_ == Mode::Dummy) { // renderer_dummy.rs:3-5
		std::memset(out, 0, (size_t)batch.out_bytes());
		return;
	}
	std::lock_guard<std::mutex> lock(mu_);
	render_view(batch.view(), out);
}

void Renderer::render_packed(PackedBatch &batch) const
{
	if (batch.n_raster == 0)
		return;
	if (mode_ == Mode::Dummy) { // renderer_dummy.rs:3-5
		std::memset(batch.out.data(), 0, (size_t)batch.out_bytes);
		return;
	}
	std::lock_guard<std::mutex> lock(mu_);
	render_view(batch.view(), batch.out.data());
}

std::optional<PbfGlyph> Renderer::render_glyph(const Face &face, uint32_t index) const
{
	TessScratch scratch;
	GlyphBatch batch;
	if (!prepare(face, index, scratch, batch))
		return std::nullopt;
	const GlyphJob &job = batch.jobs.front();
	if (!job.has_raster)
		return PbfGlyph::empty(job.id, job.advance);
	std::vector<uint8_t> bitmap((size_t)batch.out_bytes());
	render_batch(batch, bitmap.data());
	const PbfGlyphRef r = job.to_pbf(bitmap.data());
	PbfGlyph g;
	g.id = r.id;
	g.bitmap = std::move(bitmap);
	g.width = r.width;
	g.height = r.height;
	g.left = r.left;
	g.top = r.top;
	g.advance = r.advance;
	return g;
}

} // namespace vg
