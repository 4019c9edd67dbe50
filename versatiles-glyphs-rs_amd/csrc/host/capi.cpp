// capi.cpp — flat C view (include/vgfont.h) of the C++ host façade.
#include <cstring>
#include <stdexcept>

#include <unistd.h>

#include "../../../include/vgfont.h"
#include "font_manager.hpp"
#include "index_files.hpp"
#include "writers.hpp"

namespace {
thread_local std::string g_err;
int fail(const std::string &m)
{
	g_err = m;
	return -1;
}
} // namespace

struct vg_renderer {
	std::shared_ptr<vg::Renderer> r;
};
struct vg_manager {
	vg::FontManager m;
	explicit vg_manager(bool p) : m(p) {}
};
struct vg_writer {
	std::unique_ptr<vg::Writer> w;
};
struct vg_outline_batch {
	vg::OutlineBatch b;
	std::vector<uint32_t> ids, advances;
};
struct vg_glyf_batch {
	vg::GlyfPartsBatch b;
	std::vector<uint32_t> ids, advances;
};
struct vg_resident_batch {
	vg::ResidentBatch b;
	std::vector<uint32_t> ids, advances;
	uint32_t n_files = 0;
};
struct vg_glyph_batch {
	vg::PackedBatch b;
	std::vector<uint32_t> ids;
	uint32_t n_jobs = 0;
};

namespace {
struct CallbackWriter final : vg::Writer {
	vg_write_cb cb;
	void *user;
	CallbackWriter(vg_write_cb c, void *u) : cb(c), user(u) {}
	void write_directory(const std::string &p) override
	{
		if (cb && cb(user, p.c_str(), nullptr, 0, 1) != 0)
			throw std::runtime_error("writer callback failed for " + p);
	}
	void write_file(const std::string &p, const std::vector<uint8_t> &d) override { write_bytes(p, d.data(), d.size()); }
	void write_bytes(const std::string &p, const uint8_t *d, size_t n) override
	{
		if (cb && cb(user, p.c_str(), d, n, 0) != 0)
			throw std::runtime_error("writer callback failed for " + p);
	}
	void write_gather(const std::string &p, const Piece *pieces, size_t n) override
	{
		if (cb) // (the callback takes one buffer: joined by the default; the NULL sink has nothing to join for)
			vg::Writer::write_gather(p, pieces, n);
	}
};
} // namespace

extern "C" {

const char *vg_last_error(void) { return g_err.c_str(); }

vg_renderer *vg_renderer_new(int mode, int device)
{
	std::string err;
	auto r = mode == VG_MODE_DUMMY ? vg::Renderer::new_dummy() : vg::Renderer::new_precise(device, &err);
	if (!r) {
		g_err = err;
		return nullptr;
	}
	return new vg_renderer{std::move(r)};
}
vg_renderer *vg_renderer_new_multi(const int *devices, int n)
{
	if (!devices || n <= 0) {
		g_err = "vg_renderer_new_multi: no devices";
		return nullptr;
	}
	std::string err;
	auto r = vg::Renderer::new_multi(std::vector<int>(devices, devices + n), &err);
	if (!r) {
		g_err = err;
		return nullptr;
	}
	return new vg_renderer{std::move(r)};
}
int vg_renderer_device_count(const vg_renderer *r) { return (int)r->r->n_devices(); }
int vg_renderer_reduce_counters(const vg_renderer *r, uint64_t counters[3])
{
	try {
		r->r->reduce_counters(counters);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
const char *vg_renderer_reduce_path(const vg_renderer *r)
{
	static thread_local std::string keep;
	try {
		keep = r->r->reduce_path();
	} catch (const std::exception &) {
		keep.clear();
	}
	return keep.c_str();
}
void vg_renderer_add_counters(const vg_renderer *r, int lane, uint64_t blocks, uint64_t glyphs, uint64_t pixels)
{
	if (lane >= 0 && (size_t)lane < r->r->n_devices())
		r->r->device_lane((size_t)lane).add_counters(blocks, glyphs, pixels);
}
void vg_renderer_reset_counters(const vg_renderer *r) { r->r->reset_counters(); }
void vg_renderer_free(vg_renderer *r) { delete r; }
void vg_manager_reduced_counters(const vg_manager *m, uint64_t counters[3]) { std::memcpy(counters, m->m.last_reduced_counters(), 3 * sizeof(uint64_t)); }

vg_manager *vg_manager_new(int parallel) { return new vg_manager(parallel != 0); }
void vg_manager_free(vg_manager *m) { delete m; }
void vg_manager_set_device_front_end(vg_manager *m, int on) { m->m.set_device_front_end(on != 0); }
void vg_manager_set_union_outlines(vg_manager *m, int on) { m->m.set_union_outlines(on != 0); }
void vg_manager_union_stats(const vg_manager *m, uint64_t *seen, uint64_t *rebuilt, uint64_t *identity, uint64_t *over_limit)
{
	const uint64_t *s = m->m.union_stats();
	if (seen)
		*seen = s[0] + s[1] + s[2] + s[3];
	if (rebuilt)
		*rebuilt = s[1];
	if (identity)
		*identity = s[0];
	if (over_limit)
		*over_limit = s[2];
}
void vg_manager_set_in_place_pbf(vg_manager *m, int on) { m->m.set_in_place_pbf(on != 0); }
void vg_manager_set_glyf_on_device(vg_manager *m, int on) { m->m.set_glyf_on_device(on != 0); }
void vg_manager_set_resident_fonts(vg_manager *m, int on) { m->m.set_resident_fonts(on != 0); }
void vg_renderer_set_resident_budget(vg_renderer *r, uint64_t bytes_per_device) { r->r->set_resident_budget(bytes_per_device); }
long long vg_renderer_preload_fonts(vg_renderer *r, const vg_manager *m)
{
	try {
		return (long long)m->m.preload_resident_fonts(*r->r);
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_resident_stats(const vg_manager *m, vg_resident_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_resident_stats{t.resident_groups, t.resident_fonts_uploaded, t.resident_font_bytes, t.resident_block_bytes};
	return 0;
}
void vg_manager_set_resident_commands(vg_manager *m, int mode) { m->m.set_resident_commands(mode); }
int vg_manager_command_stats(const vg_manager *m, vg_command_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_command_stats{t.command_groups, t.command_fonts_uploaded, t.command_font_bytes, t.command_block_bytes};
	return 0;
}
void vg_manager_set_mixed_stores(vg_manager *m, int on) { m->m.set_mixed_stores(on != 0); }
int vg_manager_mixed_stats(const vg_manager *m, vg_mixed_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_mixed_stats{t.mixed_groups, t.mixed_glyf_fonts, t.mixed_command_fonts, t.mixed_block_bytes};
	return 0;
}
void vg_manager_set_charstrings_on_device(vg_manager *m, int on) { m->m.set_charstrings_on_device(on == 2 ? 2 : (on != 0 ? 1 : 0)); }
int vg_manager_charstring_stats(const vg_manager *m, vg_charstring_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_charstring_stats{t.charstring_fonts_decoded, t.charstring_font_bytes, t.charstring_fallbacks};
	return 0;
}
int vg_manager_charstring_preload_stats(const vg_manager *m, vg_charstring_stats *out)
{
	const vg::RenderTimings &t = m->m.last_preload_counts();
	*out = vg_charstring_stats{t.charstring_fonts_decoded, t.charstring_font_bytes, t.charstring_fallbacks};
	return 0;
}
void vg_manager_set_resident_families(vg_manager *m, int on) { m->m.set_resident_families(on != 0); }
int vg_manager_family_stats(const vg_manager *m, vg_family_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_family_stats{t.family_groups, t.families_uploaded, t.family_bytes, t.family_block_bytes};
	return 0;
}
void vg_manager_set_family_tables_on_device(vg_manager *m, int on) { m->m.set_family_tables_on_device(on != 0); }
void vg_manager_set_glyf_tables_on_device(vg_manager *m, int on) { m->m.set_glyf_tables_on_device(on != 0); }
void vg_manager_set_gvar_on_device(vg_manager *m, int on) { m->m.set_gvar_on_device(on != 0); }
int vg_manager_gvar_stats(const vg_manager *m, vg_gvar_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_gvar_stats{t.gvar_fonts_built, t.gvar_font_bytes, t.gvar_fallbacks};
	return 0;
}
int vg_manager_glyf_table_stats(const vg_manager *m, vg_glyf_table_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_glyf_table_stats{t.glyf_tables_built, t.glyf_table_bytes, t.glyf_table_fallbacks};
	return 0;
}
void vg_manager_set_glyf_tables_batched(vg_manager *m, int on) { m->m.set_glyf_tables_batched(on != 0); }
int vg_manager_glyf_table_batch_stats(const vg_manager *m, vg_glyf_table_batch_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_glyf_table_batch_stats{t.glyf_table_batch_calls, t.glyf_table_batch_faces};
	return 0;
}
int vg_manager_family_table_stats(const vg_manager *m, vg_family_table_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_family_table_stats{t.family_tables_built, t.family_table_fallbacks};
	return 0;
}
int vg_manager_family_plane_stats(const vg_manager *m, vg_family_plane_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_family_plane_stats{t.family_census_calls, t.plane_families_built, t.plane_families_stated, t.plane_family_planes};
	return 0;
}
void vg_manager_set_lane_form(vg_manager *m, int form) { m->m.set_lane_form(form < 0 || form > 2 ? -1 : form); }
void vg_manager_set_threads(vg_manager *m, unsigned threads, unsigned blocks_per_batch)
{
	m->m.set_threads(threads);
	if (blocks_per_batch)
		m->m.set_batch_blocks(blocks_per_batch);
}

int vg_manager_add_font_with_name(vg_manager *m, const char *name, const char *const *paths, int n)
{
	std::vector<std::string> ps(paths, paths + n);
	std::string err;
	return m->m.add_font_with_name(name, ps, &err) ? 0 : fail(err);
}
int vg_manager_add_font_data(vg_manager *m, const char *name, const uint8_t *data, size_t len)
{
	std::string err;
	return m->m.add_font_data(name, std::vector<uint8_t>(data, data + len), &err) ? 0 : fail(err);
}
int vg_manager_add_font_instance(vg_manager *m, const char *name, const uint8_t *data, size_t len, const char *const *axis_tags,
                                 const float *values, int n)
{
	try {
		if (!m || !name || (!data && len) || n < 0 || (n && (!axis_tags || !values)))
			return fail("vg_manager_add_font_instance: bad argument");
		std::vector<std::array<char, 4>> tags;
		for (int i = 0; i < n; i++) {
			if (!axis_tags[i] || std::strlen(axis_tags[i]) != 4)
				return fail("vg_manager_add_font_instance: an axis tag is four characters");
			std::array<char, 4> t;
			std::memcpy(t.data(), axis_tags[i], 4);
			tags.push_back(t);
		}
		std::string err;
		return m->m.add_font_instance(name, std::vector<uint8_t>(data, data + len), tags, std::vector<float>(values, values + n), &err) ? 0 : fail(err);
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_add_font_instance_normalized(vg_manager *m, const char *name, const uint8_t *data, size_t len, const int16_t *coords, int n)
{
	try {
		if (!m || !name || (!data && len) || n < 0 || (n && !coords))
			return fail("vg_manager_add_font_instance_normalized: bad argument");
		std::string err;
		return m->m.add_font_instance_normalized(name, std::vector<uint8_t>(data, data + len), std::vector<int16_t>(coords, coords + n), &err) ? 0 : fail(err);
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_add_font_named_instances(vg_manager *m, const uint8_t *data, size_t len, char (*ids)[VG_FONT_ID_MAX], int cap)
{
	try {
		if (!m || (!data && len) || cap < 0 || (cap && !ids))
			return fail("vg_manager_add_font_named_instances: bad argument");
		std::string err;
		std::vector<std::string> made;
		if (!m->m.add_font_named_instances(std::vector<uint8_t>(data, data + len), made, &err))
			return fail(err);
		for (int k = 0; k < cap && (size_t)k < made.size(); k++) {
			const size_t n = std::min(made[(size_t)k].size(), (size_t)VG_FONT_ID_MAX - 1);
			std::memcpy(ids[k], made[(size_t)k].data(), n);
			ids[k][n] = 0;
		}
		return (int)made.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
void vg_manager_set_scan_named_instances(vg_manager *m, int on) { m->m.set_scan_named_instances(on != 0); }
void vg_manager_set_gvar_batched(vg_manager *m, int on) { m->m.set_gvar_batched(on != 0); }
int vg_manager_gvar_batch_stats(const vg_manager *m, vg_gvar_batch_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_gvar_batch_stats{t.gvar_batch_calls, t.gvar_batch_faces};
	return 0;
}
void vg_manager_set_charstrings_batched(vg_manager *m, int on) { m->m.set_charstrings_batched(on != 0); }
int vg_manager_charstring_batch_stats(const vg_manager *m, vg_charstring_batch_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_charstring_batch_stats{t.charstring_batch_calls, t.charstring_batch_faces};
	return 0;
}
void vg_manager_set_family_tables_batched(vg_manager *m, int on) { m->m.set_family_tables_batched(on != 0); }
int vg_manager_family_batch_stats(const vg_manager *m, vg_family_batch_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_family_batch_stats{t.family_batch_calls, t.family_batch_families};
	return 0;
}
int vg_manager_instance_group(const vg_manager *m, const char *font_id, char (*ids)[VG_FONT_ID_MAX], int cap)
{
	try {
		if (!m || !font_id || cap < 0 || (cap && !ids))
			return fail("vg_manager_instance_group: bad argument");
		const std::vector<std::string> group = m->m.instance_group(font_id);
		for (int k = 0; k < cap && (size_t)k < group.size(); k++) {
			const size_t n = std::min(group[(size_t)k].size(), (size_t)VG_FONT_ID_MAX - 1);
			std::memcpy(ids[k], group[(size_t)k].data(), n);
			ids[k][n] = 0;
		}
		return (int)group.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
void vg_manager_set_gvar_advances(vg_manager *m, int on) { m->m.set_gvar_advances(on != 0); }
int vg_manager_gvar_advance_stats(const vg_manager *m, vg_gvar_advance_stats *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_gvar_advance_stats{m->m.gvar_advance_faces(), t.gvar_advance_builds, t.gvar_advance_fallbacks};
	return 0;
}
namespace {
// file `file_index` of a font id (nullptr and g_err: none)
const vg::Face *face_of(const vg_manager *m, const char *font_id, int file_index, const char *me)
{
	if (!m || !font_id || file_index < 0) {
		g_err = std::string(me) + ": bad argument";
		return nullptr;
	}
	auto it = m->m.fonts().find(font_id);
	if (it == m->m.fonts().end() || (size_t)file_index >= it->second.files().size()) {
		g_err = std::string("unknown font id ") + font_id + ", or a file index past its files";
		return nullptr;
	}
	return &it->second.files()[(size_t)file_index]->face();
}
} // namespace
int vg_manager_font_position(const vg_manager *m, const char *font_id, int file_index, int16_t *coords, int cap)
{
	try {
		const vg::Face *f = face_of(m, font_id, file_index, "vg_manager_font_position");
		if (!f)
			return -1;
		if (!f->at_position())
			return 0;
		for (int i = 0; coords && i < cap && (size_t)i < f->coords().size(); i++)
			coords[i] = f->coords()[(size_t)i];
		return (int)f->coords().size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_font_hor_advances(const vg_manager *m, const char *font_id, int file_index, uint16_t *advances, int cap)
{
	try {
		const vg::Face *f = face_of(m, font_id, file_index, "vg_manager_font_hor_advances");
		if (!f)
			return -1;
		if (advances && cap > 0) {
			const std::vector<uint16_t> a = f->hor_advances((uint32_t)cap);
			std::copy(a.begin(), a.end(), advances);
		}
		return (int)f->number_of_glyphs();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_font_gvar_advance_deltas(const vg_manager *m, const char *font_id, int file_index, float *delta, uint8_t *state, int cap)
{
	try {
		const vg::Face *f = face_of(m, font_id, file_index, "vg_manager_font_gvar_advance_deltas");
		if (!f)
			return -1;
		if (!f->placed_by_gvar())
			return fail(std::string("refused: font ") + font_id + ": not a glyf face placed by gvar");
		for (int g = 0; g < cap && g <= 0xFFFF; g++) {
			float d = 0.0f;
			const uint8_t s = f->gvar_advance_delta((uint16_t)g, d);
			if (delta)
				delta[g] = d;
			if (state)
				state[g] = s;
		}
		return (int)f->number_of_glyphs();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_font_variation_axes(const uint8_t *data, size_t len, char (*tags)[4], float *min, float *def, float *max, int cap)
{
	try {
		std::vector<vg::VariationAxis> axes;
		if ((!data && len) || !vg::read_variation_axes(data, len, axes))
			return fail("no readable fvar table");
		for (int i = 0; i < cap && (size_t)i < axes.size(); i++) {
			if (tags)
				std::memcpy(tags[i], axes[i].tag, 4);
			if (min)
				min[i] = axes[i].min;
			if (def)
				def[i] = axes[i].def;
			if (max)
				max[i] = axes[i].max;
		}
		return (int)axes.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_font_named_instances(const uint8_t *data, size_t len, uint16_t *name_id, float *coords, int cap_instances, int n_axes)
{
	try {
		std::vector<vg::VariationAxis> axes;
		std::vector<vg::NamedInstance> inst;
		if ((!data && len) || !vg::read_variation_axes(data, len, axes, &inst))
			return fail("no readable fvar table");
		if ((size_t)n_axes != axes.size())
			return fail("vg_font_named_instances: n_axes is not the number of the file's axes");
		for (int k = 0; k < cap_instances && (size_t)k < inst.size(); k++) {
			if (name_id)
				name_id[k] = inst[k].name_id;
			if (coords)
				std::copy(inst[k].coords.begin(), inst[k].coords.end(), coords + (size_t)k * axes.size());
		}
		return (int)inst.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_add_path(vg_manager *m, const char *path)
{
	std::string err;
	return m->m.add_path(path, &err) ? 0 : fail(err);
}
int vg_manager_shard_glyphs(const vg_manager *m, const char *font_id, uint32_t world, uint8_t *owner, double *cost)
{
	vg::GlyphShard sh;
	std::string err;
	if (!m->m.shard_glyphs(font_id, world, sh, &err))
		return fail(err);
	if (owner)
		std::memcpy(owner, sh.owner.data(), sh.owner.size());
	if (cost)
		std::memcpy(cost, sh.cost.data(), sh.cost.size() * sizeof(double));
	return 0;
}

int vg_manager_plan_lanes(vg_manager *m, const char *font_id, uint32_t world, uint8_t *owner, uint32_t *n_split_blocks, double *est_max_over_mean)
{
	try {
		std::vector<uint8_t> own;
		uint32_t n_split = 0;
		std::string err;
		if (!m->m.plan_lanes(font_id, world, own, n_split, est_max_over_mean, &err))
			return fail(err);
		if (owner)
			std::memcpy(owner, own.data(), own.size());
		if (n_split_blocks)
			*n_split_blocks = n_split;
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_manager_set_glyph_shard(vg_manager *m, uint32_t rank, uint32_t world)
{
	try {
		m->m.set_glyph_shard(rank, world);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

long vg_pbf_merge(const uint8_t *const *parts, const size_t *lens, int n, uint8_t *out, size_t cap)
{
	try {
		std::vector<std::pair<const uint8_t *, size_t>> ps;
		for (int i = 0; i < n; i++)
			ps.emplace_back(parts[i], lens[i]);
		const std::vector<uint8_t> v = vg::merge_pbf_partials(ps);
		if (out && cap >= v.size())
			std::memcpy(out, v.data(), v.size());
		return (long)v.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

long vg_pbf_concat(const uint8_t *const *parts, const size_t *lens, int n, uint8_t *out, size_t cap)
{
	try {
		std::vector<std::pair<const uint8_t *, size_t>> ps;
		for (int i = 0; i < n; i++)
			ps.emplace_back(parts[i], lens[i]);
		const std::vector<uint8_t> v = vg::concat_pbf_partials(ps);
		if (out && cap >= v.size())
			std::memcpy(out, v.data(), v.size());
		return (long)v.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_manager_scan(vg_manager *m, const char *path)
{
	std::string err;
	return m->m.scan(path, &err) ? 0 : fail(err);
}

static long copy_out(const std::string &s, char *out, size_t cap, bool nul)
{
	if (out && cap) {
		const size_t n = std::min(nul ? cap - 1 : cap, s.size());
		std::memcpy(out, s.data(), n);
		if (nul)
			out[n] = 0;
	}
	return (long)(s.size() + (nul ? 1 : 0));
}

long vg_manager_font_ids(const vg_manager *m, char *out, size_t cap)
{
	std::string s;
	for (const auto &kv : m->m.fonts()) {
		if (!s.empty())
			s.push_back('\n');
		s += kv.first;
	}
	return copy_out(s, out, cap, true);
}

long vg_manager_font_file_names(const vg_manager *m, const char *font_id, char *out, size_t cap)
{
	auto it = m->m.fonts().find(font_id);
	if (it == m->m.fonts().end())
		return fail(std::string("unknown font id ") + font_id);
	std::string s;
	for (const auto &f : it->second.files()) {
		if (!s.empty())
			s.push_back('\n');
		s += f->metadata().name;
	}
	return copy_out(s, out, cap, true);
}

int vg_parse_font_name(const char *family, const char *ps_name, char *family_out, size_t cap, char *style_out,
                       uint16_t *weight_out, char *width_out)
{
	const vg::ParsedFontName p = vg::parse_font_name(family ? family : "", ps_name ? ps_name : "");
	copy_out(p.family, family_out, cap, true);
	if (style_out)
		copy_out(p.style, style_out, 16, true);
	if (width_out)
		copy_out(p.width, width_out, 16, true);
	if (weight_out)
		*weight_out = p.weight;
	return (int)p.family.size();
}

long vg_manager_generate_name(const vg_manager *m, const char *font_id, int file_index, char *out, size_t cap)
{
	auto it = m->m.fonts().find(font_id);
	if (it == m->m.fonts().end() || file_index < 0 || (size_t)file_index >= it->second.files().size())
		return fail("unknown font id / file index");
	return copy_out(it->second.files()[(size_t)file_index]->metadata().generate_name(), out, cap, true);
}

long vg_encode_codeblocks(const uint32_t *codepoints, size_t n, char *out, size_t cap)
{
	return copy_out(vg::encode_codeblocks(std::vector<uint32_t>(codepoints, codepoints + n)), out, cap, true);
}

long vg_manager_index_json(const vg_manager *m, uint8_t *out, size_t cap)
{
	const auto v = vg::build_index_json(m->m);
	return copy_out(std::string(v.begin(), v.end()), (char *)out, cap, false);
}

long vg_manager_families_json(const vg_manager *m, uint8_t *out, size_t cap)
{
	try {
		const auto v = vg::build_font_families_json(m->m);
		return copy_out(std::string(v.begin(), v.end()), (char *)out, cap, false);
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

vg_writer *vg_writer_new_tar_path(const char *path, int64_t mtime)
{
	std::FILE *f = std::fopen(path, "wb");
	if (!f) {
		g_err = std::string("cannot create ") + path;
		return nullptr;
	}
	return new vg_writer{std::unique_ptr<vg::Writer>(new vg::TarWriter(f, true, mtime))};
}

vg_writer *vg_writer_new_tar_fd(int fd, int64_t mtime)
{
	const int dupfd = ::dup(fd); // fclose() of our stream must not close the caller's descriptor
	std::FILE *f = dupfd >= 0 ? ::fdopen(dupfd, "wb") : nullptr;
	if (!f) {
		if (dupfd >= 0)
			::close(dupfd);
		g_err = "cannot open descriptor " + std::to_string(fd) + " for writing";
		return nullptr;
	}
	return new vg_writer{std::unique_ptr<vg::Writer>(new vg::TarWriter(f, true, mtime))};
}

vg_writer *vg_writer_new_dir(const char *folder) { return new vg_writer{std::unique_ptr<vg::Writer>(new vg::FileWriter(folder))}; }

int vg_writer_write_file(vg_writer *w, const char *path, const uint8_t *data, size_t len)
{
	try {
		w->w->write_file(path, std::vector<uint8_t>(data, data + len));
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_writer_write_directory(vg_writer *w, const char *path)
{
	try {
		w->w->write_directory(path);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_writer_finish(vg_writer *w)
{
	try {
		w->w->finish();
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

void vg_writer_free(vg_writer *w) { delete w; }

int vg_manager_render_glyphs_to(vg_manager *m, vg_renderer *r, vg_writer *w)
{
	try {
		m->m.render_glyphs(*w->w, *r->r);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_manager_write_index_json(const vg_manager *m, vg_writer *w)
{
	try {
		m->m.write_index_json(*w->w);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_manager_write_families_json(const vg_manager *m, vg_writer *w)
{
	try {
		m->m.write_families_json(*w->w);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_name_to_id(const char *name, char *out, size_t cap)
{
	const std::string id = vg::name_to_id(name);
	if (out && cap) {
		const size_t n = std::min(cap - 1, id.size());
		std::memcpy(out, id.data(), n);
		out[n] = 0;
	}
	return (int)id.size();
}
int vg_manager_block_counts(const vg_manager *m, const char *font_id, uint32_t counts[256])
{
	auto it = m->m.fonts().find(font_id);
	if (it == m->m.fonts().end())
		return fail(std::string("unknown font id ") + font_id);
	const auto blocks = it->second.get_blocks();
	for (size_t i = 0; i < 256; i++)
		counts[i] = (uint32_t)blocks[i].len();
	return 0;
}

int vg_manager_set_supplementary_planes(vg_manager *m, int on)
{
	try {
		m->m.set_supplementary_planes(on != 0);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_supplementary_blocks(const vg_manager *m, const char *font_id, uint32_t *starts, uint32_t *counts, int cap)
{
	auto it = m->m.fonts().find(font_id);
	if (it == m->m.fonts().end())
		return fail(std::string("unknown font id ") + font_id);
	const std::vector<vg::GlyphBlock> &blocks = it->second.blocks();
	int n = 0;
	for (size_t i = vg::kBmpBlocks; i < blocks.size(); i++, n++)
		if (n < cap) {
			if (starts)
				starts[n] = blocks[i].start_index;
			if (counts)
				counts[n] = (uint32_t)blocks[i].len();
		}
	return n;
}

int vg_manager_render_glyphs(vg_manager *m, vg_renderer *r, vg_write_cb cb, void *user)
{
	try {
		CallbackWriter w(cb, user);
		m->m.render_glyphs(w, *r->r);
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_render_blocks(vg_manager *m, vg_renderer *r, const char *font_id, const uint32_t *starts, int n,
                             vg_write_cb cb, void *user)
{
	try {
		CallbackWriter w(cb, user);
		m->m.render_blocks(w, *r->r, font_id, std::vector<uint32_t>(starts, starts + n));
		return 0;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}
int vg_manager_timings(const vg_manager *m, vg_timings *out)
{
	const vg::RenderTimings &t = m->m.last_timings();
	*out = vg_timings{t.tessellate_s, t.pack_s, t.device_s, t.encode_s, t.write_s, t.total_s, t.blocks,
	                  t.glyphs,       t.rasters,  t.pixels,   t.segments, t.pbf_bytes,  t.glyf_groups, t.glyf_fallbacks,
	                  t.fe_groups,    t.fe_max_group_glyphs};
	return 0;
}
long vg_manager_render_block(vg_manager *m, vg_renderer *r, const char *font_id, uint32_t start, uint8_t *out,
                             size_t cap)
{
	try {
		auto it = m->m.fonts().find(font_id);
		if (it == m->m.fonts().end())
			return fail(std::string("unknown font id ") + font_id);
		if (start % 256 || (start > 0xFF00 && !m->m.supplementary_planes()))
			return fail("block start must be a multiple of 256 below 65536");
		const auto blocks = it->second.get_blocks();
		const vg::GlyphBlock *block = vg::FontWrapper::find_block(blocks, start);
		if (!block) // (a supplementary start the font id does not populate)
			return fail("bad block start " + std::to_string(start));
		const std::vector<uint8_t> pbf = block->render(font_id, *r->r);
		if (out && pbf.size() <= cap)
			std::memcpy(out, pbf.data(), pbf.size());
		return (long)pbf.size();
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

int vg_render_glyph(vg_renderer *r, const vg_manager *m, const char *font_id, int file_index, uint32_t index,
                    vg_pbf_glyph *out, uint8_t *bitmap, size_t cap)
{
	try {
		auto it = m->m.fonts().find(font_id);
		if (it == m->m.fonts().end())
			return fail(std::string("unknown font id ") + font_id);
		const auto &files = it->second.files();
		if (file_index < 0 || (size_t)file_index >= files.size())
			return fail("file index out of range");
		const auto g = r->r->render_glyph(files[(size_t)file_index]->face(), index);
		if (!g)
			return 0;
		out->id = g->id;
		out->has_bitmap = g->bitmap ? 1 : 0;
		out->width = g->width;
		out->height = g->height;
		out->left = g->left;
		out->top = g->top;
		out->advance = g->advance;
		out->bitmap_len = g->bitmap ? (uint32_t)g->bitmap->size() : 0;
		if (g->bitmap) {
			if (g->bitmap->size() > cap)
				return fail("bitmap buffer too small");
			std::memcpy(bitmap, g->bitmap->data(), g->bitmap->size());
		}
		return 1;
	} catch (const std::exception &e) {
		return fail(e.what());
	}
}

vg_glyph_batch *vg_manager_build_batch(vg_manager *m, const char *font_id)
{
	try {
		auto *b = new vg_glyph_batch();
		std::string err;
		if (!m->m.build_batch(font_id, b->b, b->ids, b->n_jobs, &err)) {
			delete b;
			g_err = err;
			return nullptr;
		}
		return b;
	} catch (const std::exception &e) {
		g_err = e.what();
		return nullptr;
	}
}
int vg_glyph_batch_view(const vg_glyph_batch *b, vgsdf_batch *view, const uint32_t **ids, uint32_t *n_jobs)
{
	*view = b->b.view();
	if (ids)
		*ids = b->ids.data();
	if (n_jobs)
		*n_jobs = b->n_jobs;
	return 0;
}
void vg_glyph_batch_free(vg_glyph_batch *b) { delete b; }

vg_outline_batch *vg_manager_record_outlines(const vg_manager *m, const char *font_id)
{
	try {
		auto *b = new vg_outline_batch();
		std::string err;
		if (!m->m.record_outlines(font_id, b->b, &err)) {
			delete b;
			g_err = err;
			return nullptr;
		}
		for (const vg::GlyphJob &j : b->b.jobs) {
			b->ids.push_back(j.id);
			b->advances.push_back(j.advance);
		}
		return b;
	} catch (const std::exception &e) {
		g_err = e.what();
		return nullptr;
	}
}
int vg_outline_batch_view(const vg_outline_batch *b, vgsdf_outlines *view, const uint32_t **ids, const uint32_t **advances)
{
	*view = b->b.view();
	if (ids)
		*ids = b->ids.data();
	if (advances)
		*advances = b->advances.data();
	return 0;
}
void vg_outline_batch_free(vg_outline_batch *b) { delete b; }

vg_glyf_batch *vg_manager_record_glyf_parts(const vg_manager *m, const char *font_id)
{
	try {
		auto *b = new vg_glyf_batch();
		std::string err;
		if (!m->m.record_glyf_parts(font_id, b->b, &err)) {
			delete b;
			g_err = err;
			return nullptr;
		}
		for (const vg::GlyphJob &j : b->b.jobs) {
			b->ids.push_back(j.id);
			b->advances.push_back(j.advance);
		}
		return b;
	} catch (const std::exception &e) {
		g_err = e.what();
		return nullptr;
	}
}
int vg_glyf_batch_view(const vg_glyf_batch *b, vgsdf_outlines_glyf *view, const uint32_t **ids, const uint32_t **advances)
{
	static_assert(sizeof(vg::GlyfPart) == sizeof(vgsdf_glyf_part), "same record");
	const vg::GlyfPartsBatch &g = b->b;
	view->n_glyphs = (uint32_t)g.jobs.size();
	view->n_parts = (uint32_t)g.parts.size();
	view->n_bytes = (uint32_t)g.bytes.size();
	view->cmd_off = g.slot_off.data();
	view->parts = reinterpret_cast<const vgsdf_glyf_part *>(g.parts.data());
	view->bytes = g.bytes.data();
	view->scale = g.scale.data();
	view->shift_x = g.shift_x.data();
	view->pbf_pre = nullptr;
	view->pbf_fix = nullptr;
	if (ids)
		*ids = b->ids.data();
	if (advances)
		*advances = b->advances.data();
	return 0;
}
void vg_glyf_batch_free(vg_glyf_batch *b) { delete b; }

int vg_manager_resident_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_desc *desc)
{
	try {
		std::string err;
		const vg::ResidentTable *t = file_index < 0 ? nullptr : m->m.resident_table(font_id, (size_t)file_index, &err);
		if (!t || !desc) {
			g_err = err.empty() ? "vg_manager_resident_font_desc: bad argument" : err;
			return -1;
		}
		desc->n_glyph_ids = (uint32_t)t->leaf_off.size() - 1;
		desc->n_leaves = (uint32_t)t->leaves.size();
		desc->n_bytes = (uint32_t)t->bytes.size();
		desc->leaf_off = t->leaf_off.data();
		desc->leaves = reinterpret_cast<const vgsdf_glyf_part *>(t->leaves.data());
		desc->bytes = t->bytes.data();
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
vg_resident_batch *vg_manager_record_resident(const vg_manager *m, const char *font_id)
{
	try {
		auto b = std::make_unique<vg_resident_batch>();
		std::string err;
		if (!m->m.record_resident(font_id, b->b, &err)) {
			g_err = err;
			return nullptr;
		}
		for (const vg::GlyphJob &j : b->b.jobs) {
			b->ids.push_back(j.id);
			b->advances.push_back(j.advance);
		}
		b->n_files = (uint32_t)m->m.fonts().at(font_id).files().size();
		return b.release();
	} catch (const std::exception &e) {
		g_err = e.what();
		return nullptr;
	}
}
int vg_manager_command_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_cmds_desc *desc)
{
	try {
		std::string err;
		const vg::CommandTable *t = file_index < 0 || !m || !font_id ? nullptr : m->m.command_table(font_id, (size_t)file_index, &err);
		if (!t || !desc) {
			g_err = err.empty() ? "vg_manager_command_font_desc: bad argument" : err;
			return -1;
		}
		desc->n_glyph_ids = (uint32_t)t->cmd_off.size() - 1;
		desc->n_cmds = (uint32_t)t->kinds.size();
		desc->n_floats = (uint32_t)t->coords.size();
		desc->cmd_off = t->cmd_off.data();
		desc->dat_off = t->dat_off.data();
		desc->kinds = t->kinds.data();
		desc->coords = t->coords.data();
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_charstring_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_charstrings_desc *desc)
{
	try {
		std::string err;
		const vg::CharstringTable *t = file_index < 0 || !m || !font_id ? nullptr : m->m.charstring_table(font_id, (size_t)file_index, &err);
		if (!t || !desc) {
			g_err = err.empty() ? "vg_manager_charstring_font_desc: bad argument" : err;
			return -1;
		}
		desc->n_glyph_ids = (uint32_t)t->cs_off.size() - 1;
		desc->n_bytes = (uint32_t)t->bytes.size();
		desc->bytes = t->bytes.data();
		desc->cs_off = t->cs_off.data();
		desc->n_gsubrs = (uint32_t)t->gsubr_off.size() - 1;
		desc->gsubr_off = t->gsubr_off.data();
		desc->n_fds = t->n_fds;
		desc->lsubr_first = t->lsubr_first.data();
		desc->lsubr_off = t->lsubr_off.data();
		desc->fd_of = t->fd_of.empty() ? nullptr : t->fd_of.data();
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_charstring2_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_charstrings2_desc *desc)
{
	try {
		std::string err;
		const vg::CharstringTable *t = file_index < 0 || !m || !font_id ? nullptr : m->m.charstring2_table(font_id, (size_t)file_index, &err);
		if (!t || !desc) {
			g_err = err.empty() ? "vg_manager_charstring2_font_desc: bad argument" : err;
			return -1;
		}
		vgsdf_font_charstrings_desc &cs = desc->charstrings;
		cs.n_glyph_ids = (uint32_t)t->cs_off.size() - 1;
		cs.n_bytes = (uint32_t)t->bytes.size();
		cs.bytes = t->bytes.data();
		cs.cs_off = t->cs_off.data();
		cs.n_gsubrs = (uint32_t)t->gsubr_off.size() - 1;
		cs.gsubr_off = t->gsubr_off.data();
		cs.n_fds = t->n_fds;
		cs.lsubr_first = t->lsubr_first.data();
		cs.lsubr_off = t->lsubr_off.data();
		cs.fd_of = nullptr;
		desc->n_sets = (uint32_t)t->set_ok.size();
		desc->n_factors = (uint32_t)t->factors.size();
		desc->set_ok = t->set_ok.data();
		desc->set_off = t->set_off.data();
		desc->factors = t->factors.data();
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_charstring2_fonts_desc(const vg_manager *m, const char *font_id, vgsdf_fonts_charstrings2_desc *desc)
{
	try {
		std::string err;
		vg::FontManager::Charstring2Group group;
		if (!m || !font_id || !desc || !m->m.charstring2_group(font_id, group, &err)) {
			g_err = err.empty() ? "vg_manager_charstring2_fonts_desc: bad argument" : err;
			return -1;
		}
		const vg::CharstringTable *t = group.first;
		vgsdf_font_charstrings_desc &cs = desc->face.charstrings;
		cs.n_glyph_ids = (uint32_t)t->cs_off.size() - 1;
		cs.n_bytes = (uint32_t)t->bytes.size();
		cs.bytes = t->bytes.data();
		cs.cs_off = t->cs_off.data();
		cs.n_gsubrs = (uint32_t)t->gsubr_off.size() - 1;
		cs.gsubr_off = t->gsubr_off.data();
		cs.n_fds = t->n_fds;
		cs.lsubr_first = t->lsubr_first.data();
		cs.lsubr_off = t->lsubr_off.data();
		cs.fd_of = nullptr;
		desc->face.n_sets = (uint32_t)t->set_ok.size();
		desc->face.n_factors = (uint32_t)t->factors.size();
		desc->face.set_ok = t->set_ok.data();
		desc->face.set_off = t->set_off.data();
		desc->face.factors = group.factors;
		desc->n_positions = group.n_positions;
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
vg_resident_batch *vg_manager_record_resident_commands(const vg_manager *m, const char *font_id)
{
	try {
		auto b = std::make_unique<vg_resident_batch>();
		std::string err;
		if (!m || !font_id || !m->m.record_resident_commands(font_id, b->b, &err)) {
			g_err = err.empty() ? "vg_manager_record_resident_commands: bad argument" : err;
			return nullptr;
		}
		for (const vg::GlyphJob &j : b->b.jobs) {
			b->ids.push_back(j.id);
			b->advances.push_back(j.advance);
		}
		b->n_files = (uint32_t)m->m.fonts().at(font_id).files().size();
		return b.release();
	} catch (const std::exception &e) {
		g_err = e.what();
		return nullptr;
	}
}
int vg_manager_family_desc(const vg_manager *m, const char *font_id, vg_family_view *view)
{
	try {
		std::string err;
		const vg::FontManager::FamilyTable *t = m && font_id && view ? m->m.family_table(font_id, &err) : nullptr;
		if (!t) {
			g_err = err.empty() ? "vg_manager_family_desc: bad argument" : err;
			return -1;
		}
		view->n_entries = (uint32_t)t->code_point.size();
		view->n_files = (uint32_t)t->n_files;
		view->code_point = t->code_point.data();
		view->font_of = t->font_of.data();
		view->glyph_id = t->glyph_id.data();
		view->advance = t->advance.data();
		view->scale = t->scale.data();
		view->shift_x = t->shift_x.data();
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_family_tables_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_face_tables *desc)
{
	try {
		if (!m || !font_id || !desc || file_index < 0) {
			g_err = "vg_manager_family_tables_desc: bad argument";
			return -1;
		}
		auto it = m->m.fonts().find(font_id);
		if (it == m->m.fonts().end() || (size_t)file_index >= it->second.files().size()) {
			g_err = std::string("unknown font id ") + font_id + ", or a file index past its files";
			return -1;
		}
		const vg::FamilyTables &t = it->second.files()[(size_t)file_index]->face().family_tables();
		if (!t.ok) {
			g_err = std::string("refused: font ") + font_id +
			        (t.hvar_refused ? ": an HVAR advance map of a format other than 0 and 1 or outside the table, or more word deltas than regions"
			                        : ": a cmap subtable whose segments or groups are not regular");
			return -1;
		}
		desc->cmap = t.cmap, desc->cmap_len = t.cmap_len;
		desc->hmtx = t.hmtx, desc->hmtx_len = t.hmtx_len;
		desc->units_per_em = t.units_per_em, desc->num_glyphs = t.num_glyphs, desc->num_hmetrics = t.num_hmetrics;
		desc->n_subtables = (uint16_t)t.subtable_off.size();
		desc->subtable_off = t.subtable_off.data();
		desc->subtable_format = t.subtable_format.data();
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_family_variation_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_face_variation *desc)
{
	try {
		if (!m || !font_id || !desc || file_index < 0) {
			g_err = "vg_manager_family_variation_desc: bad argument";
			return -1;
		}
		auto it = m->m.fonts().find(font_id);
		if (it == m->m.fonts().end() || (size_t)file_index >= it->second.files().size()) {
			g_err = std::string("unknown font id ") + font_id + ", or a file index past its files";
			return -1;
		}
		const vg::FamilyTables &t = it->second.files()[(size_t)file_index]->face().family_tables();
		if (!t.ok) {
			g_err = std::string("refused: font ") + font_id +
			        (t.hvar_refused ? ": an HVAR advance map of a format other than 0 and 1 or outside the table, or more word deltas than regions"
			                        : ": a cmap subtable whose segments or groups are not regular");
			return -1;
		}
		*desc = vgsdf_face_variation{t.hvar, t.hvar_len, t.hvar_store, t.hvar_map, t.hvar ? t.region_scalars.data() : nullptr,
		                             t.hvar ? (uint32_t)t.region_scalars.size() : 0u};
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_font_tables_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_tables_desc *desc)
{
	try {
		if (!m || !font_id || !desc || file_index < 0) {
			g_err = "vg_manager_font_tables_desc: bad argument";
			return -1;
		}
		auto it = m->m.fonts().find(font_id);
		if (it == m->m.fonts().end() || (size_t)file_index >= it->second.files().size()) {
			g_err = std::string("unknown font id ") + font_id + ", or a file index past its files";
			return -1;
		}
		const vg::FontTables t = it->second.files()[(size_t)file_index]->face().font_tables();
		if (!t.ok) {
			g_err = std::string("refused: font ") + font_id + ": no glyf outlines";
			return -1;
		}
		desc->num_glyphs = t.num_glyphs, desc->loca_entries = t.loca_entries, desc->loca_long = t.loca_long;
		desc->n_loca_bytes = t.n_loca_bytes, desc->n_glyf_bytes = t.n_glyf_bytes;
		desc->loca = t.loca, desc->glyf = t.glyf;
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_gvar_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_gvar_desc *desc)
{
	try {
		if (!m || !font_id || !desc || file_index < 0) {
			g_err = "vg_manager_gvar_font_desc: bad argument";
			return -1;
		}
		auto it = m->m.fonts().find(font_id);
		if (it == m->m.fonts().end() || (size_t)file_index >= it->second.files().size()) {
			g_err = std::string("unknown font id ") + font_id + ", or a file index past its files";
			return -1;
		}
		const vg::GvarTables t = it->second.files()[(size_t)file_index]->face().gvar_tables();
		if (!t.ok) {
			g_err = std::string("refused: font ") + font_id + ": not a glyf face placed by gvar";
			return -1;
		}
		desc->tables.num_glyphs = t.tables.num_glyphs, desc->tables.loca_entries = t.tables.loca_entries, desc->tables.loca_long = t.tables.loca_long;
		desc->tables.n_loca_bytes = t.tables.n_loca_bytes, desc->tables.n_glyf_bytes = t.tables.n_glyf_bytes;
		desc->tables.loca = t.tables.loca, desc->tables.glyf = t.tables.glyf;
		desc->gvar = t.gvar, desc->gvar_len = t.gvar_len, desc->n_axes = t.n_axes, desc->coords = t.coords;
		return 0;
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_manager_family_gvar_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_gvar_desc *desc)
{
	try {
		const vg::Face *f = desc ? face_of(m, font_id, file_index, "vg_manager_family_gvar_desc") : nullptr;
		if (!f) {
			if (!desc)
				g_err = "vg_manager_family_gvar_desc: bad argument";
			return -1;
		}
		*desc = vgsdf_font_gvar_desc{};
		if (!f->advances_by_gvar())
			return 0; // (all zero: the face takes nothing from gvar)
		return vg_manager_gvar_font_desc(m, font_id, file_index, desc);
	} catch (const std::exception &e) {
		g_err = e.what();
		return -1;
	}
}
int vg_resident_batch_view(const vg_resident_batch *b, vg_resident_view *view)
{
	if (!b || !view)
		return -1;
	view->n_glyphs = (uint32_t)b->b.jobs.size();
	view->n_files = b->n_files;
	view->font_of = b->b.font_of.data();
	view->glyph_id = b->b.glyph_id.data();
	view->scale = b->b.scale.data();
	view->shift_x = b->b.shift_x.data();
	view->ids = b->ids.data();
	view->advances = b->advances.data();
	return 0;
}
void vg_resident_batch_free(vg_resident_batch *b) { delete b; }

long vg_pbf_encode(const char *name, const char *range, const vg_pbf_glyph *glyphs, const uint8_t *const *bitmaps,
                   int n, uint8_t *out, size_t cap)
{
	std::vector<vg::PbfGlyphRef> refs((size_t)n);
	static const uint8_t kEmpty = 0;
	for (int i = 0; i < n; i++) {
		vg::PbfGlyphRef &r = refs[(size_t)i];
		r.id = glyphs[i].id;
		if (glyphs[i].has_bitmap) {
			r.bitmap = bitmaps && bitmaps[i] ? bitmaps[i] : &kEmpty;
			r.bitmap_len = glyphs[i].bitmap_len;
		}
		r.width = glyphs[i].width;
		r.height = glyphs[i].height;
		r.left = glyphs[i].left;
		r.top = glyphs[i].top;
		r.advance = glyphs[i].advance;
	}
	const std::vector<uint8_t> pbf = vg::PbfGlyphs::encode(name, range, std::move(refs));
	if (out && pbf.size() <= cap)
		std::memcpy(out, pbf.data(), pbf.size());
	return (long)pbf.size();
}

} // extern "C"
