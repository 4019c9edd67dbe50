// front_end_dispatch.cpp — FontManager's dispatcher with the DEVICE front-end: host threads only look glyphs up and record
// their outline commands (or name the glyphs, or their code-point ranges); flattening, ring rules, scale/shift, bbox and the
// raster run on the GPU, one submission per group of blocks.  Which form a group takes (fe_candidates, fe_record), the recorders,
// the stores and families they name, assembly, encode / write and the pipelined run (run_tasks_device_front_end).
#include "font_manager.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "font_manager_internal.hpp"

namespace vg {

// units of host work of a group: 64-code-point slices of its non-empty blocks, in task order
void FontManager::fe_make_slices(const std::vector<Todo> &tasks, FeGroup &G, uint32_t per_slice)
{
	G.slices.clear();
	G.slice_ci.clear();
	for (size_t t = G.g0; t < G.g1; t++) {
		if (tasks[t].block.is_empty())
			continue;
		for (uint32_t c = 0; c < GLYPH_BLOCK_SIZE; c += per_slice) {
			OSlice s;
			s.task = (uint32_t)t;
			G.slices.push_back(s);
			G.slice_ci.push_back(c);
		}
	}
}

// jobs of a task are contiguous in the merged batch: [task_g0[t], task_g0[t + 1]); the first glyph of a block leaves room
// for the block's file + fontstack header in front of its entry
void FontManager::fe_layout_common(const std::vector<Todo> &tasks, FeGroup &G)
{
	MergedOutlines &m = G.m;
	const std::vector<OSlice> &slices = G.slices;
	G.task_g0.assign(G.g1 - G.g0 + 1, G.n_jobs);
	size_t t_next = 0;
	for (size_t i = 0; i < slices.size(); i++)
		for (; t_next <= slices[i].task - G.g0; t_next++)
			G.task_g0[t_next] = slices[i].g_job;
	if (m.pbf_pre)
		for (size_t t = G.g0; t < G.g1; t++) {
			const uint32_t a = G.task_g0[t - G.g0], b = G.task_g0[t - G.g0 + 1];
			if (a < b)
				m.pbf_pre[a] = kPbfHeadRoom + pbf_block_fields(tasks[t].name->size(), tasks[t].block.range().size());
		}
}

namespace {

bool trace_pack()
{
	static const bool on = std::getenv("VG_TRACE_PACK") != nullptr;
	return on;
}

// a store or a family that this call put on the device (bytes != 0), counted
void count_upload(uint64_t bytes, uint64_t &n, uint64_t &sum)
{
	if (bytes)
		n++, sum += bytes;
}

} // namespace

// The host half of a group in the forms that record glyph by glyph: the workers record 64-code-point slices of the group's
// non-empty blocks into their own batches, a serial pass over the slices says where each lands in the merged batch, and a second
// fork copies them there in task order (jobs, commands / parts and bytes of a slice are contiguous in its worker's batch).
// A Form says what differs between the forms:
//   Local, local(w)   the worker's batch the form fills;   kLight: its forks are light ones (thread_pool.hpp)
//   recorder(l)       a callable (file, code point) that records one glyph into l; made per slice, so it may keep state
//   count(l, s)       notes in s what its jobs [job0, job1) added to l, in g_cmd, g_dat, g_byte (offsets after the serial pass)
//   fits(workers)     after recording: false = not a batch for the device in this form (nothing is laid out then)
//   layout(m, ...)    places the arrays of the merged batch for the summed counts
//   copy(m, s, l)     copies the slice's payload; returns what job() needs of the slice
//   job(m, s, l, base, j, g)   what job j of l, glyph g of the merged batch, has beyond the lines every form has
// t0: when the caller began recording the group.
template <class Form> bool FontManager::fe_record_slices(const std::vector<Todo> &tasks, FeGroup &G, Form form, double t0)
{
	constexpr uint32_t kSlice = 64;
	ThreadPool &tp = pool();
	std::vector<OSlice> &slices = G.slices;
	fe_make_slices(tasks, G, kSlice);
	for (Worker &w : workers_)
		form.local(w).clear();
	tp.run(slices.size(), [&](size_t i, unsigned wid) {
		OSlice &s = slices[i];
		typename Form::Local &l = form.local(workers_[wid]);
		s.worker = wid;
		s.job0 = (uint32_t)l.jobs.size();
		const GlyphBlock &blk = tasks[s.task].block;
		auto record = form.recorder(l);
		for (uint32_t ci = G.slice_ci[i]; ci < G.slice_ci[i] + kSlice; ci++)
			if (const FontFileEntry *f = blk.glyphs[ci])
				record(f, blk.start_index + ci);
		s.job1 = (uint32_t)l.jobs.size();
		form.count(l, s);
	}, Form::kLight);
	const double t1 = now_s();
	timings_.tessellate_s += t1 - t0;
	if (!form.fits(workers_))
		return false;

	uint32_t n_jobs = 0, n_cmd = 0, n_dat = 0, n_byte = 0;
	for (OSlice &s : slices) {
		const uint32_t c = s.g_cmd, d = s.g_dat, b = s.g_byte; // (the slice's counts, until here)
		s.g_job = n_jobs, s.g_cmd = n_cmd, s.g_dat = n_dat, s.g_byte = n_byte;
		n_jobs += s.job1 - s.job0, n_cmd += c, n_dat += d, n_byte += b;
	}
	G.n_jobs = n_jobs;
	MergedOutlines &m = G.m;
	m.jobs.resize(n_jobs);
	G.in_place = in_place_pbf_;
	const bool trace = Form::kTracePack && trace_pack(); // (the clock is read for the trace line only)
	const double tp0 = trace ? now_s() : 0;
	form.layout(m, n_jobs, n_cmd, n_dat, n_byte, G.in_place);
	const double tp1 = trace ? now_s() : 0;
	tp.run(slices.size(), [&](size_t i, unsigned) {
		const OSlice &s = slices[i];
		const typename Form::Local &l = form.local(workers_[s.worker]);
		const auto base = form.copy(m, s, l);
		for (uint32_t j = s.job0; j < s.job1; j++) {
			const uint32_t g = s.g_job + (j - s.job0);
			m.jobs[g] = l.jobs[j];
			m.scale[g] = l.scale[j];
			m.shift_x[g] = l.shift_x[j];
			if (m.pbf_fix) {
				m.pbf_pre[g] = 0;
				m.pbf_fix[g] = pbf_fix_of(l.jobs[j].id, l.jobs[j].advance);
			}
			form.job(m, s, l, base, j, g);
		}
	}, Form::kLight);
	const double tp2 = trace ? now_s() : 0;
	fe_layout_common(tasks, G);
	if (trace)
		std::fprintf(stderr, "[pack] slices %zu jobs %u parts %u bytes %u: sums %.1f us, layout %.1f, copy fork %.1f, common %.1f\n", slices.size(), n_jobs,
		             n_dat, n_byte, (tp0 - t1) * 1e6, (tp1 - tp0) * 1e6, (tp2 - tp1) * 1e6, (now_s() - tp2) * 1e6);
	timings_.pack_s += now_s() - t1;
	return true;
}

// The host reader's commands, recorded by the workers in the compact upload form itself (a kind byte per command + the
// coordinates its kind carries): merging is a copy.  g_cmd counts commands, g_dat coordinates.
struct FontManager::PackedForm {
	using Local = PackedOutlineBatch;
	static constexpr bool kLight = false, kTracePack = false;
	static Local &local(Worker &w) { return w.olocal; }
	static auto recorder(Local &l) { return [&l](const FontFileEntry *f, uint32_t cp) { Renderer::record(f->face(), cp, l); }; }
	static void count(const Local &l, OSlice &s) { s.g_cmd = l.cmd_off[s.job1] - l.cmd_off[s.job0], s.g_dat = l.dat_off[s.job1] - l.dat_off[s.job0]; }
	static bool fits(const std::vector<Worker> &) { return true; }
	static void layout(MergedOutlines &m, uint32_t n_jobs, uint32_t n_cmds, uint32_t n_floats, uint32_t, bool with_pbf)
	{
		m.layout(n_jobs, n_cmds, n_floats, with_pbf);
		m.cmd_off[0] = m.dat_off[0] = 0;
	}
	struct Base { uint32_t cmd, dat; }; // the slice's first command / coordinate in its worker's batch
	static Base copy(MergedOutlines &m, const OSlice &s, const Local &l)
	{
		const uint32_t lc0 = l.cmd_off[s.job0], lc1 = l.cmd_off[s.job1], ld0 = l.dat_off[s.job0], ld1 = l.dat_off[s.job1];
		if (lc1 > lc0)
			std::memcpy(m.kinds + s.g_cmd, l.kinds.data() + lc0, lc1 - lc0);
		if (ld1 > ld0)
			std::memcpy(m.coords + s.g_dat, l.coords.data() + ld0, sizeof(float) * (ld1 - ld0));
		return Base{lc0, ld0};
	}
	static void job(MergedOutlines &m, const OSlice &s, const Local &l, Base b, uint32_t j, uint32_t g)
	{
		m.cmd_off[g + 1] = s.g_cmd + (l.cmd_off[j + 1] - b.cmd);
		m.dat_off[g + 1] = s.g_dat + (l.dat_off[j + 1] - b.dat);
	}
};

// The group's glyphs for the device's glyf decoder (vgsdf_outlines_glyf): the workers look every glyph up and copy the
// arrays of its simple glyphs as they stand — no point is decoded on the host (0.56 us of CPU per glyph with the
// reader's recorder, ~0.1 here).  g_cmd counts command slots, g_dat parts.
struct FontManager::GlyfForm {
	using Local = GlyfPartsBatch;
	static constexpr bool kLight = true, kTracePack = true;
	static Local &local(Worker &w) { return w.plocal; }
	static auto recorder(Local &l) { return [&l](const FontFileEntry *f, uint32_t cp) { Renderer::record_parts(f->face(), cp, l); }; }
	// first byte of `part` (the end of the store behind the last one)
	static uint32_t byte_at(const Local &l, uint32_t part) { return part < l.parts.size() ? l.parts[part].byte_off : (uint32_t)l.bytes.size(); }
	static void count(const Local &l, OSlice &s)
	{
		s.g_cmd = l.slot_off[s.job1] - l.slot_off[s.job0];
		s.g_dat = l.part_off[s.job1] - l.part_off[s.job0];
		s.g_byte = byte_at(l, l.part_off[s.job1]) - byte_at(l, l.part_off[s.job0]);
	}
	// a worker's batch stays below 2^26 bytes / slots (Face::glyph_parts); the merged batch must fit 32-bit offsets too
	static bool fits(const std::vector<Worker> &workers)
	{
		uint64_t bytes = 0, slots = 0, n_p = 0;
		bool overflow = false;
		for (const Worker &w : workers) {
			overflow = overflow || w.plocal.overflow;
			bytes += w.plocal.bytes.size();
			slots += w.plocal.slots;
			n_p += w.plocal.parts.size();
		}
		return !(overflow || bytes >= (1ull << 31) || slots >= (1ull << 31) || n_p >= (1ull << 31));
	}
	static void layout(MergedOutlines &m, uint32_t n_jobs, uint32_t, uint32_t n_parts, uint32_t n_bytes, bool with_pbf)
	{
		m.layout_glyf(n_jobs, n_parts, n_bytes, with_pbf);
		m.cmd_off[0] = 0;
	}
	struct Base { uint32_t slot; }; // the slice's first command slot in its worker's batch
	static Base copy(MergedOutlines &m, const OSlice &s, const Local &l)
	{
		const uint32_t p0 = l.part_off[s.job0], p1 = l.part_off[s.job1], s0 = l.slot_off[s.job0];
		const uint32_t b0 = byte_at(l, p0), b1 = byte_at(l, p1);
		if (b1 > b0)
			std::memcpy(m.glyf_bytes + s.g_byte, l.bytes.data() + b0, b1 - b0);
		for (uint32_t k = p0; k < p1; k++) {
			vgsdf_glyf_part q;
			static_assert(sizeof q == sizeof l.parts[k], "same record");
			std::memcpy(&q, &l.parts[k], sizeof q);
			q.byte_off = s.g_byte + (l.parts[k].byte_off - b0);
			q.cmd_at = s.g_cmd + (l.parts[k].cmd_at - s0);
			m.parts[s.g_dat + (k - p0)] = q;
		}
		return Base{s0};
	}
	static void job(MergedOutlines &m, const OSlice &s, const Local &l, Base b, uint32_t j, uint32_t g) { m.cmd_off[g + 1] = s.g_cmd + (l.slot_off[j + 1] - b.slot); }
};

// The group's glyphs by name (vgsdf_outlines_resident): the faces' outlines are on the device, so a worker's share per
// glyph is the cmap and hmtx lookups — no composite is walked, no font byte copied.
struct FontManager::NamedForm {
	using Local = ResidentBatch;
	static constexpr bool kLight = true, kTracePack = false;
	const std::vector<std::pair<const FontFileEntry *, uint16_t>> &index; // sorted by address: a face -> its place in m.fonts
	bool commands; // the block of command fonts (else: the glyf form's, which fonts of both kinds take as well)
	static Local &local(Worker &w) { return w.rlocal; }
	auto recorder(Local &l) const
	{
		return [this, &l, prev = (const FontFileEntry *)nullptr, prev_at = (uint16_t)0](const FontFileEntry *f, uint32_t cp) mutable {
			if (f != prev) {
				prev = f;
				prev_at = std::lower_bound(index.begin(), index.end(), std::make_pair(f, (uint16_t)0))->second;
			}
			Renderer::record_resident(f->face(), prev_at, cp, l);
		};
	}
	static void count(const Local &, OSlice &) {}
	static bool fits(const std::vector<Worker> &) { return true; }
	void layout(MergedOutlines &m, uint32_t n_jobs, uint32_t, uint32_t, uint32_t, bool with_pbf) const { m.layout_resident(n_jobs, with_pbf, commands); }
	struct Base {};
	static Base copy(MergedOutlines &, const OSlice &, const Local &) { return Base{}; }
	static void job(MergedOutlines &m, const OSlice &, const Local &l, Base, uint32_t j, uint32_t g) { m.glyph_id[g] = l.glyph_id[j], m.font_of[g] = l.font_of[j]; }
};

void FontManager::fe_record_packed(const std::vector<Todo> &tasks, FeGroup &G) { (void)fe_record_slices(tasks, G, PackedForm{}, now_s()); }

bool FontManager::fe_record_glyf(const std::vector<Todo> &tasks, FeGroup &G) { return fe_record_slices(tasks, G, GlyfForm{}, now_s()); }

bool FontManager::fe_record_named(const std::vector<Todo> &tasks, FeGroup &G, const Renderer &renderer, int lane, StoreKind kind)
{
	const double t0 = now_s();
	const bool commands = kind == StoreKind::Commands;
	G.mixed_glyf_stores = G.mixed_command_stores = 0;
	MergedOutlines &m = G.m;
	// the faces of the group's fonts (tasks of one font follow each other) and their device copies
	m.fonts.clear();
	std::vector<std::pair<const FontFileEntry *, uint16_t>> index;
	const std::string *last = nullptr;
	for (size_t t = G.g0; t < G.g1; t++) {
		if (tasks[t].name == last)
			continue;
		last = tasks[t].name;
		auto it = fonts().find(*last);
		if (it == fonts().end())
			return false;
		if (kind == StoreKind::Glyf || (kind == StoreKind::Mixed && !glyf_refused_.count(&it->first)))
			glyf_stores_batched(renderer, lane, it->second, timings_);
		for (const auto &file : it->second.files()) {
			if (m.fonts.size() >= 0xFFFF)
				return false;
			bool glyf = kind == StoreKind::Glyf;
			const vgsdf_font *f = kind == StoreKind::Mixed ? file_store(renderer, lane, it->first, file->face(), timings_, &glyf)
			                      : commands               ? command_store(renderer, lane, file->face(), timings_)
			                                               : glyf_store(renderer, lane, file->face(), timings_);
			if (!f)
				return false;
			(glyf ? G.mixed_glyf_stores : G.mixed_command_stores)++;
			index.emplace_back(file.get(), (uint16_t)m.fonts.size());
			m.fonts.push_back(f);
		}
	}
	if (kind == StoreKind::Mixed && G.mixed_glyf_stores == 0) // (nothing to mix: the command forms take the group, as without the switch)
		return false;
	std::sort(index.begin(), index.end());
	return fe_record_slices(tasks, G, NamedForm{index, commands}, t0);
}

const vgsdf_font *FontManager::glyf_store(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const
{
	uint64_t uploaded = 0;
	const vgsdf_font *f = nullptr;
	if (glyf_tables_on_device_) {
		bool refused = false, over_budget = false, built = false;
		f = renderer.font_from_tables(lane, face.resident_serial(), face.font_tables(), &uploaded, &refused, &over_budget, &built);
		if (refused)
			counts.glyf_table_fallbacks++;
		if (over_budget)
			return nullptr; // (the host's table would make a font of the same leaves over the same budget: it is not built for that)
		if (built)
			counts.glyf_tables_built++, counts.glyf_table_bytes += uploaded;
	}
	if (!f)
		f = renderer.resident_font(lane, face.resident_table(), &uploaded);
	if (f)
		count_upload(uploaded, counts.resident_fonts_uploaded, counts.resident_font_bytes);
	return f;
}

void FontManager::glyf_stores_batched(const Renderer &renderer, int lane, const FontWrapper &font, RenderTimings &counts) const
{
	if (!glyf_tables_on_device_ || !glyf_tables_batched_)
		return;
	std::vector<Renderer::TablesJob> faces;
	for (const auto &file : font.files())
		if (file->face().has_glyf_form())
			faces.push_back(Renderer::TablesJob{file->face().resident_serial(), file->face().font_tables()});
	std::vector<Renderer::TablesOutcome> outcomes;
	renderer.fonts_from_tables(lane, faces, outcomes, &counts.glyf_table_batch_calls, &counts.glyf_table_batch_faces);
	for (const Renderer::TablesOutcome &o : outcomes) { // (as glyf_store counts what font_from_tables says)
		if (o.refused)
			counts.glyf_table_fallbacks++;
		if (o.built) {
			counts.glyf_tables_built++, counts.glyf_table_bytes += o.uploaded;
			count_upload(o.uploaded, counts.resident_fonts_uploaded, counts.resident_font_bytes);
		}
	}
}

void FontManager::gvar_stores_batched(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const
{
	if (!gvar_batched_)
		return;
	const InstanceGroup *group = instance_group_of(face);
	if (!group || group->faces.size() < 2)
		return; // (a face with bytes of its own: its own call)
	std::vector<Renderer::GvarJob> faces;
	for (const Face *f : group->faces)
		faces.push_back(Renderer::GvarJob{f->command_serial(), f->gvar_tables()});
	std::vector<Renderer::TablesOutcome> outcomes;
	renderer.gvar_fonts(lane, faces, outcomes, &counts.gvar_batch_calls, &counts.gvar_batch_faces);
	for (const Renderer::TablesOutcome &o : outcomes) { // (as command_store counts what gvar_font says)
		if (o.refused)
			counts.gvar_fallbacks++;
		if (o.built) {
			count_upload(o.uploaded, counts.gvar_fonts_built, counts.gvar_font_bytes);
			count_upload(o.uploaded, counts.command_fonts_uploaded, counts.command_font_bytes);
		}
	}
}

void FontManager::charstring2_stores_batched(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const
{
	if (!charstrings_batched_ || charstrings_on_device_ < 2)
		return;
	const InstanceGroup *group = instance_group_of(face);
	if (!group || group->faces.size() < 2)
		return; // (a face with bytes of its own: its own call)
	std::vector<Renderer::Charstring2Job> faces;
	for (const Face *f : group->faces) {
		const CharstringTable &t = f->charstring2_table();
		faces.push_back(Renderer::Charstring2Job{t.serial, &t});
	}
	std::vector<Renderer::TablesOutcome> outcomes;
	renderer.charstring2_fonts(lane, faces, outcomes, &counts.charstring_batch_calls, &counts.charstring_batch_faces);
	for (const Renderer::TablesOutcome &o : outcomes) { // (as command_store counts what charstring_font says)
		if (o.refused)
			counts.charstring_fallbacks++;
		if (o.built) {
			count_upload(o.uploaded, counts.charstring_fonts_decoded, counts.charstring_font_bytes);
			count_upload(o.uploaded, counts.command_fonts_uploaded, counts.command_font_bytes);
		}
	}
}

void FontManager::families_batched(const Renderer &renderer, int lane, const FontWrapper &font, StoreKind kind, RenderTimings &counts) const
{
	if (!family_tables_on_device_ || !family_tables_batched_ || kind == StoreKind::Glyf || font.files().size() != 1)
		return; // (a placed face has no glyf form: its family is over command stores, alone or mixed)
	const InstanceGroup *group = instance_group_of(font.files()[0]->face());
	if (!group || group->faces.size() < 2)
		return;
	std::vector<Renderer::FamilyJob> jobs;
	for (size_t k = 0; k < group->faces.size(); k++) {
		const auto it = fonts().find(group->ids[k]);
		if (it == fonts().end() || it->second.files().size() != 1)
			continue; // (two records merged into one id: a family of two files, the single way)
		const Face &face = *group->faces[k];
		const FamilyTables &t = face.family_tables();
		if (!t.ok)
			continue; // (the single way refuses it and counts that)
		FamilyTable *shell = family_shell(it->first, 1);
		{
			std::lock_guard<std::mutex> lock(family_mu_of());
			if (shell->refused)
				continue;
		}
		const vgsdf_font *store = command_store(renderer, lane, face, counts); // (gvar_stores_batched inside, as today)
		if (!store)
			continue; // (over the budget)
		jobs.push_back(Renderer::FamilyJob{shell->serial, store, &t, face.advances_by_gvar() ? face.gvar_tables() : GvarTables{}});
	}
	if (jobs.size() < 2)
		return;
	std::vector<Renderer::FamilyOutcome> outcomes;
	renderer.families_from_tables(lane, jobs, kind == StoreKind::Mixed ? Renderer::kFamilyMixed : Renderer::kFamilyCommands, outcomes,
	                              &counts.family_batch_calls, &counts.family_batch_families);
	for (size_t i = 0; i < outcomes.size(); i++) { // (as device_family counts what family_from_tables says)
		const Renderer::FamilyOutcome &o = outcomes[i];
		if (o.refused) {
			counts.family_table_fallbacks++;
			counts.gvar_advance_fallbacks += jobs[i].gvar.ok;
		}
		if (o.built) {
			count_upload(o.uploaded, counts.families_uploaded, counts.family_bytes);
			counts.family_tables_built++;
			counts.gvar_advance_builds += jobs[i].gvar.ok;
		}
	}
}

const vgsdf_font *FontManager::command_store(const Renderer &renderer, int lane, const Face &face, RenderTimings &counts) const
{
	uint64_t uploaded = 0;
	const vgsdf_font *f = nullptr;
	// (1: `CFF ` version 1 faces; 2: CFF2 faces as well)
	const CharstringTable *cs = charstrings_on_device_ >= 1 && face.charstring_table().ok ? &face.charstring_table() : nullptr;
	if (!cs && charstrings_on_device_ >= 2 && face.charstring2_table().ok)
		cs = &face.charstring2_table();
	if (cs) {
		if (cs->cff2)
			charstring2_stores_batched(renderer, lane, face, counts);
		bool refused = false, over_budget = false;
		f = renderer.charstring_font(lane, *cs, &uploaded, &refused, &over_budget);
		if (refused)
			counts.charstring_fallbacks++;
		if (over_budget)
			return nullptr; // (the host's table would make the same store, over the same budget: it is not built for that)
		if (f)
			count_upload(uploaded, counts.charstring_fonts_decoded, counts.charstring_font_bytes);
	}
	if (!f && gvar_on_device_ && face.placed_by_gvar()) {
		gvar_stores_batched(renderer, lane, face, counts);
		bool refused = false, over_budget = false;
		f = renderer.gvar_font(lane, face.command_serial(), face.gvar_tables(), &uploaded, &refused, &over_budget);
		if (refused)
			counts.gvar_fallbacks++;
		if (over_budget)
			return nullptr; // (the host's table would make the same store, over the same budget: it is not built for that)
		if (f)
			count_upload(uploaded, counts.gvar_fonts_built, counts.gvar_font_bytes);
	}
	if (!f)
		f = renderer.command_font(lane, face.command_table(), &uploaded);
	if (f)
		count_upload(uploaded, counts.command_fonts_uploaded, counts.command_font_bytes);
	return f;
}

const vgsdf_font *FontManager::file_store(const Renderer &renderer, int lane, const std::string &font_id, const Face &face,
                                          RenderTimings &counts, bool *glyf) const
{
	*glyf = false;
	if (face.has_glyf_form() && !glyf_refused_.count(&font_id))
		if (const vgsdf_font *f = glyf_store(renderer, lane, face, counts)) {
			*glyf = true;
			return f;
		}
	return command_store(renderer, lane, face, counts);
}

bool FontManager::may_mix(const std::vector<Todo> &tasks, size_t g0, size_t g1) const
{
	const std::string *last = nullptr;
	for (size_t t = g0; t < g1; t++) {
		if (tasks[t].name == last)
			continue;
		last = tasks[t].name;
		auto it = fonts().find(*last);
		if (it == fonts().end() || glyf_refused_.count(&it->first))
			continue;
		for (const auto &file : it->second.files())
			if (file->face().has_glyf_form())
				return true;
	}
	return false;
}

const vgsdf_family *FontManager::device_family(const Renderer &renderer, int lane, const std::string &font_id, const FontWrapper &font,
                                               StoreKind kind, const FamilyTable **table, RenderTimings &counts, uint32_t *glyf_stores,
                                               uint32_t *command_stores, uint32_t plane) const
{
	const bool commands = kind == StoreKind::Commands;
	const int family_kind = kind == StoreKind::Mixed ? Renderer::kFamilyMixed : commands ? Renderer::kFamilyCommands : Renderer::kFamilyGlyf;
	// (a supplementary plane: the device builds a STATIC font id's family; a font id with a placed face takes the host's table,
	// since the _var and _gvar constructors are plane 0)
	bool on_device = family_tables_on_device_ && font.files().size() <= 0x10000;
	for (const auto &file : font.files())
		on_device = on_device && !(plane && file->face().at_position());
	const FamilyTable *ft = on_device ? nullptr : family_table(font_id, nullptr, plane);
	if (!ft && !on_device)
		return nullptr;
	std::vector<const vgsdf_font *> stores;
	if (kind == StoreKind::Glyf || (kind == StoreKind::Mixed && !glyf_refused_.count(&font_id)))
		glyf_stores_batched(renderer, lane, font, counts);
	if (on_device && plane == 0)
		families_batched(renderer, lane, font, kind, counts); // (the lookup below then finds the family)
	for (const auto &file : font.files()) {
		bool glyf = kind == StoreKind::Glyf;
		const vgsdf_font *f = kind == StoreKind::Mixed ? file_store(renderer, lane, font_id, file->face(), counts, &glyf)
		                      : commands               ? command_store(renderer, lane, file->face(), counts)
		                                               : (file->face().has_glyf_form() ? glyf_store(renderer, lane, file->face(), counts) : nullptr);
		if (!f)
			return nullptr;
		stores.push_back(f);
		if (uint32_t *n = glyf ? glyf_stores : command_stores)
			++*n;
	}
	uint64_t uploaded = 0;
	if (on_device) {
		// the faces' descriptions (no code point is looked up) and the device's build; a refusal of either sends the font id the
		// host's way below, for good
		FamilyTable *shell = family_shell(font_id, font.files().size(), plane);
		std::vector<vgsdf_face_tables> descs;
		std::vector<vgsdf_face_variation> variation; // filled once a face at a position with an HVAR is met
		// the faces whose advances follow gvar's phantom points (Face::advances_by_gvar): their tables beside `variation`
		std::vector<vgsdf_font_gvar_desc> gvar_descs;
		std::vector<const vgsdf_font_gvar_desc *> gvar;
		gvar_descs.reserve(font.files().size());
		for (const auto &file : font.files()) {
			const FamilyTables &t = file->face().family_tables();
			if (!t.ok) {
				std::lock_guard<std::mutex> lock(family_mu_of());
				if (!shell->refused)
					counts.family_table_fallbacks++;
				shell->refused = true;
				break;
			}
			vgsdf_face_tables d;
			d.cmap = t.cmap, d.cmap_len = t.cmap_len, d.hmtx = t.hmtx, d.hmtx_len = t.hmtx_len;
			d.units_per_em = t.units_per_em, d.num_glyphs = t.num_glyphs, d.num_hmetrics = t.num_hmetrics;
			d.n_subtables = (uint16_t)t.subtable_off.size();
			d.subtable_off = t.subtable_off.data(), d.subtable_format = t.subtable_format.data();
			descs.push_back(d);
			if (t.hvar || !variation.empty()) {
				variation.resize(descs.size(), vgsdf_face_variation{nullptr, 0, 0, 0, nullptr, 0});
				variation.back() = vgsdf_face_variation{t.hvar, t.hvar_len, t.hvar_store, t.hvar_map, t.region_scalars.data(), (uint32_t)t.region_scalars.size()};
			}
			const GvarTables g = file->face().advances_by_gvar() ? file->face().gvar_tables() : GvarTables{};
			if (g.ok || !gvar.empty()) {
				gvar.resize(descs.size(), nullptr);
				if (g.ok) {
					vgsdf_font_gvar_desc gd{};
					gd.tables.num_glyphs = g.tables.num_glyphs, gd.tables.loca_entries = g.tables.loca_entries, gd.tables.loca_long = g.tables.loca_long;
					gd.tables.n_loca_bytes = g.tables.n_loca_bytes, gd.tables.n_glyf_bytes = g.tables.n_glyf_bytes;
					gd.tables.loca = g.tables.loca, gd.tables.glyf = g.tables.glyf;
					gd.gvar = g.gvar, gd.gvar_len = g.gvar_len, gd.n_axes = g.n_axes, gd.coords = g.coords;
					gvar_descs.push_back(gd);
					gvar.back() = &gvar_descs.back();
				}
			}
		}
		// which planes are worth a device build: ONE census of the font id's tables, kept in its plane-0 shell.  (The block table
		// has already said that the plane holds a block; a plane the census finds empty — it cannot, being a superset — and a census
		// that failed leave the family to the host's table.)
		bool listed = true;
		if (plane && descs.size() == font.files().size()) {
			FamilyTable *root = family_shell(font_id, font.files().size(), 0);
			std::lock_guard<std::mutex> lock(family_mu_of());
			if (!root->census_done) {
				root->census_done = renderer.family_census(lane, descs, &root->census_planes) ? 1 : 2;
				counts.family_census_calls++;
			}
			listed = root->census_done == 1 && ((root->census_planes >> plane) & 1u);
		}
		if (descs.size() == font.files().size() && listed) {
			int refused = 0;
			bool built = false;
			const vgsdf_family *fam = renderer.family_from_tables(lane, shell->serial, descs, stores, family_kind, &uploaded, &refused, &built, variation, gvar, plane);
			if (built && plane)
				counts.plane_families_built++, counts.plane_family_planes |= 1ull << plane;
			if (refused == 1) {
				counts.family_table_fallbacks++;
				counts.gvar_advance_fallbacks += !gvar_descs.empty();
			}
			if (built) {
				count_upload(uploaded, counts.families_uploaded, counts.family_bytes);
				counts.family_tables_built++;
				counts.gvar_advance_builds += !gvar_descs.empty();
			}
			if (fam) {
				std::lock_guard<std::mutex> lock(family_mu_of());
				if (!shell->filled) {
					renderer.family_names(lane, fam, shell->code_point, shell->advance);
					shell->filled = true;
				}
			}
			if (fam || !refused) { // (no family and no refusal: over the budget, as the host's way would be)
				if (table)
					*table = shell;
				return fam;
			}
		}
		uploaded = 0;
		ft = family_table(font_id, nullptr, plane);
		if (!ft)
			return nullptr;
	}
	const Renderer::FamilyArrays fa{ft->serial, &ft->code_point, &ft->font_of, &ft->glyph_id, &ft->advance, &ft->scale, &ft->shift_x, ft->plane};
	const vgsdf_family *fam = renderer.family(lane, fa, stores, family_kind, &uploaded);
	if (fam)
		count_upload(uploaded, counts.families_uploaded, counts.family_bytes);
	if (fam && uploaded && plane)
		counts.plane_families_stated++, counts.plane_family_planes |= 1ull << plane;
	if (table)
		*table = ft;
	return fam;
}

// The group as code-point ranges of its font ids' resident families (vgsdf_outlines_submit_ranges): no glyph is touched — per
// task two bisections of the family's code points; the device names the glyphs and, in place, writes their PBF entries.
bool FontManager::fe_record_ranges(const std::vector<Todo> &tasks, FeGroup &G, const Renderer &renderer, int lane, StoreKind kind)
{
	const double t0 = now_s();
	G.mixed_glyf_stores = G.mixed_command_stores = 0;
	FeGroup::Ranges &R = G.ranges;
	R.clear();
	const size_t nb = G.g1 - G.g0;
	std::vector<uint32_t> task_g0(nb + 1, 0);
	const std::string *last = nullptr;
	const FamilyTable *ft = nullptr;
	uint32_t n_jobs = 0, last_plane = 0;
	for (size_t t = G.g0; t < G.g1; t++) {
		const uint32_t plane = tasks[t].block.start_index >> 16; // (a family per font id AND plane)
		if (tasks[t].name != last || plane != last_plane) {
			auto it = fonts().find(*tasks[t].name);
			if (it == fonts().end() || R.families.size() >= 0xFFFF)
				return false;
			const vgsdf_family *fam = device_family(renderer, lane, it->first, it->second, kind, &ft, timings_, &G.mixed_glyf_stores, &G.mixed_command_stores, plane);
			if (!fam)
				return false;
			last = tasks[t].name, last_plane = plane;
			R.families.push_back(fam);
			R.tables.push_back(ft);
		}
		const GlyphBlock &blk = tasks[t].block;
		task_g0[t - G.g0] = n_jobs;
		R.task_r0.push_back((uint32_t)R.first.size());
		if (blk.len() == 0)
			continue;
		const auto &cp = ft->code_point; // (low halves, as the tasks' first and last)
		auto add = [&](uint32_t a, uint32_t b, uint32_t room) { // code points [a, b] of the block
			const auto lo = std::lower_bound(cp.begin(), cp.end(), (uint16_t)a), hi = std::upper_bound(cp.begin(), cp.end(), (uint16_t)b);
			R.family_of.push_back((uint16_t)(R.families.size() - 1));
			R.first.push_back((uint16_t)a);
			R.last.push_back((uint16_t)b);
			R.pre.push_back(room);
			R.entry_first.push_back((uint32_t)(lo - cp.begin()));
			n_jobs += (uint32_t)(hi - lo);
			return (uint32_t)(hi - lo);
		};
		const uint32_t room = (uint32_t)(kPbfHeadRoom + pbf_block_fields(tasks[t].name->size(), blk.range().size()));
		const uint32_t s = blk.start_index & 0xFFFFu;
		const auto lo = std::lower_bound(cp.begin(), cp.end(), (uint16_t)s), hi = std::upper_bound(cp.begin(), cp.end(), (uint16_t)(s + GLYPH_BLOCK_SIZE - 1));
		if ((size_t)(hi - lo) == blk.len()) {
			add(s, s + GLYPH_BLOCK_SIZE - 1, room);
		} else { // a block that keeps some of its glyphs (the hybrid lane plan's split): one task per run of code points it keeps
			bool first = true;
			for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE;) {
				if (!blk.glyphs[ci]) {
					ci++;
					continue;
				}
				uint32_t cj = ci;
				while (cj < GLYPH_BLOCK_SIZE && blk.glyphs[cj])
					cj++;
				if (add(s + ci, s + cj - 1, first ? room : 0u))
					first = false;
				else // (a run the family maps nothing of: no task)
					R.family_of.pop_back(), R.first.pop_back(), R.last.pop_back(), R.pre.pop_back(), R.entry_first.pop_back();
				ci = cj;
			}
		}
	}
	if (kind == StoreKind::Mixed && G.mixed_glyf_stores == 0) // (nothing to mix: the command forms take the group)
		return false;
	task_g0[nb] = n_jobs;
	R.task_r0.push_back((uint32_t)R.first.size());
	G.task_g0 = std::move(task_g0);
	G.n_jobs = n_jobs;
	G.in_place = in_place_pbf_;
	timings_.pack_s += now_s() - t0;
	return true;
}

uint64_t FontManager::preload_resident_fonts(const Renderer &renderer) const
{
	uint64_t uploaded = 0;
	preload_counts_ = RenderTimings{};
	for (size_t r = 0; r < renderer.n_devices(); r++)
		for (const auto &kv : fonts()) {
			RenderTimings batch;
			glyf_stores_batched(renderer.device_lane(r), 0, kv.second, batch);
			uploaded += batch.resident_font_bytes;
			preload_counts_.add_uploads(batch);
			for (const auto &file : kv.second.files())
				if (file->face().has_glyf_form()) {
					RenderTimings counts;
					(void)glyf_store(renderer.device_lane(r), 0, file->face(), counts);
					uploaded += counts.resident_font_bytes;
					if (glyf_tables_on_device_) // (with the switch off these uploads go into the returned total only, as they always have)
						preload_counts_.add_uploads(counts);
				}
		}
	// ... and the command stores the manager's mode would use: with 2 every face's, with 1 those of the fonts whose groups cannot
	// take a glyf form (a file without `glyf` outlines, a font refused before) — with mixed stores, of such a font the files alone
	// that get no glyf store (file_store)
	auto glyf_files_keep_glyf_stores = [this](const std::string &font_id) { return mixes() && !glyf_refused_.count(&font_id); };
	if (resident_commands_)
		for (size_t r = 0; r < renderer.n_devices(); r++)
			for (const auto &kv : fonts()) {
				bool wanted = resident_commands_ == 2 || glyf_refused_.count(&kv.first) != 0;
				for (const auto &file : kv.second.files())
					wanted = wanted || !file->face().has_glyf_form();
				if (wanted)
					for (const auto &file : kv.second.files()) {
						if (file->face().has_glyf_form() && glyf_files_keep_glyf_stores(kv.first))
							continue;
						RenderTimings counts;
						(void)command_store(renderer.device_lane(r), 0, file->face(), counts);
						uploaded += counts.command_font_bytes;
						preload_counts_.add_uploads(counts);
					}
			}
	// ... and the families over them, of the kinds of store the modes would name (with mixed stores a font id with a `glyf` file
	// goes by its glyf or its mixed family, and gets no family over command stores of all its files)
	if (resident_families_)
		for (size_t r = 0; r < renderer.n_devices(); r++)
			for (const auto &kv : fonts()) {
				bool a_glyf_file = false;
				for (const auto &file : kv.second.files())
					a_glyf_file = a_glyf_file || file->face().has_glyf_form();
				for (const StoreKind kind : {StoreKind::Glyf, StoreKind::Commands, StoreKind::Mixed})
					if (kind == StoreKind::Mixed      ? mixes()
					    : kind == StoreKind::Commands ? resident_commands_ != 0 && !(a_glyf_file && glyf_files_keep_glyf_stores(kv.first))
					                                  : resident_fonts_) {
						RenderTimings counts;
						(void)device_family(renderer.device_lane(r), 0, kv.first, kv.second, kind, nullptr, counts);
						uploaded += counts.family_bytes + counts.resident_font_bytes + counts.command_font_bytes;
						preload_counts_.add_uploads(counts);
					}
			}
	return uploaded;
}

// The order in which the forms are tried for a group: the one place that says it.  device_forms: the call may use a form other
// than the host reader's; glyf_forms: the glyf forms are on (fe_record passes them over for a group with a glyph from another
// kind of file, or of a font the decoder has refused); by_name: there is a renderer whose stores the glyphs can be named against; by_ranges: families are on
// and usable.  Wherever a group would go by glyph names its ranges are tried first.
FontManager::FormList FontManager::fe_candidates(bool device_forms, bool glyf_forms, bool by_name, bool by_ranges) const
{
	FormList c;
	auto add = [&c](bool on, GroupForm f) {
		if (on)
			c.form[c.n++] = f;
	};
	auto against_stores = [&](bool commands) {
		add(by_ranges, commands ? GroupForm::RangesCommands : GroupForm::RangesGlyf);
		add(by_name, commands ? GroupForm::NamedCommands : GroupForm::NamedGlyf);
	};
	if (device_forms) {
		if (resident_commands_ == 2) // every group against command stores
			against_stores(true);
		if (glyf_forms) {
			if (resident_fonts_)
				against_stores(false);
			add(true, GroupForm::GlyfParts);
		}
		if (resident_commands_ == 1) { // a group that took no glyf form
			if (glyf_forms && mixes()) { // ... against the store each of its files gets (fe_record: not for a group that is all `glyf`)
				add(by_ranges, GroupForm::RangesMixed);
				add(by_name, GroupForm::NamedMixed);
			}
			against_stores(true);
		}
	}
	add(true, GroupForm::Packed); // the host's reader records whatever is left
	return c;
}

void FontManager::fe_record(const std::vector<Todo> &tasks, FeGroup &G, bool allow_glyf, const Renderer *renderer, int lane)
{
	// families: not under glyph sharding, whose blocks hold a rank's share of every block
	const bool families = resident_families_ && (parent_ != nullptr || shard_world_ == 1) && renderer != nullptr;
	const FormList forms = fe_candidates(allow_glyf, glyf_on_device_, renderer != nullptr, families);
	int all_glyf = -1; // every glyph of the group comes from a `glyf` file of a font not refused; looked at when a glyf form's turn comes
	int can_mix = -1;  // ... and, when a mixed form's turn comes, whether the group is one for them
	auto group_all_glyf = [&] {
		if (all_glyf < 0) {
			all_glyf = 1;
			for (size_t t = G.g0; t < G.g1 && all_glyf; t++)
				all_glyf = tasks[t].block.all_glyf && !glyf_refused_.count(tasks[t].name);
		}
		return all_glyf != 0;
	};
	for (unsigned k = 0; k < forms.n; k++) {
		G.form = forms.form[k];
		if (G.form == GroupForm::RangesGlyf || G.form == GroupForm::NamedGlyf || G.form == GroupForm::GlyfParts) {
			(void)group_all_glyf();
			if (!all_glyf)
				continue;
		}
		if (G.form == GroupForm::RangesMixed || G.form == GroupForm::NamedMixed) {
			// a group whose glyphs all come from `glyf` files has had its turn with the glyf forms; a group without a `glyf` file
			// that could get a glyf store has nothing to mix
			if (can_mix < 0)
				can_mix = !group_all_glyf() && may_mix(tasks, G.g0, G.g1);
			if (!can_mix)
				continue;
		}
		switch (G.form) {
		case GroupForm::RangesGlyf:
		case GroupForm::RangesCommands:
		case GroupForm::RangesMixed:
			if (fe_record_ranges(tasks, G, *renderer, lane,
			                     G.form == GroupForm::RangesMixed      ? StoreKind::Mixed
			                     : G.form == GroupForm::RangesCommands ? StoreKind::Commands
			                                                           : StoreKind::Glyf))
				return;
			break;
		case GroupForm::NamedGlyf:
		case GroupForm::NamedCommands:
		case GroupForm::NamedMixed:
			if (fe_record_named(tasks, G, *renderer, lane,
			                    G.form == GroupForm::NamedMixed      ? StoreKind::Mixed
			                    : G.form == GroupForm::NamedCommands ? StoreKind::Commands
			                                                         : StoreKind::Glyf))
				return;
			break;
		case GroupForm::GlyfParts:
			if (fe_record_glyf(tasks, G))
				return;
			for (size_t t = G.g0; t < G.g1; t++) // composite fan-out past the batch bounds: the host's reader from now on
				glyf_refused_.insert(tasks[t].name);
			timings_.glyf_fallbacks++;
			break;
		case GroupForm::Packed:
			fe_record_packed(tasks, G);
			return;
		}
	}
}

// In-place assembly: the raster has stored every bitmap of the group where its block's finished PBF has it (the arena
// G.out, laid out by outline_plan from pbf_pre / pbf_fix); what is left is the ~20 bytes around each bitmap and the
// block headers, written here on the pool.  A block without a glyph of this group is encoded on its own (32 bytes).
// Every position the device reports is checked against this side's own arithmetic.
// What of the assembly needs no result of the device: the files of the blocks without a glyph of this group (211 of a
// font's 256, typically: name + range only, ~35 bytes each, written into one store — a vector per file cost more than all
// the header bytes of the font together) and the list of the others.  Runs on the calling thread between the submission and
// the wait for the front-end's results, when it has nothing else to do.
void FontManager::fe_prepare_pieces(const std::vector<Todo> &tasks, FeGroup &G)
{
	const double t3 = now_s();
	const size_t nb = G.g1 - G.g0;
	using Piece = FeGroup::Piece;
	std::vector<Piece> &piece = G.piece;
	piece.assign(nb, Piece{});
	size_t small_stride = 0;
	for (size_t i = 0; i < nb; i++)
		small_stride = std::max(small_stride, tasks[G.g0 + i].name->size() + 48);
	std::vector<uint8_t> &small = G.small;
	small.resize(nb * small_stride);
	G.busy.clear();
	auto empty_file = [&](size_t i) { // the file of a block without a glyph of this group: name + range
		const Todo &td = tasks[G.g0 + i];
		const std::string &range = td.block.range();
		uint8_t *entries = small.data() + i * small_stride + kPbfHeadRoom + pbf_block_fields(td.name->size(), range.size());
		uint8_t *file = write_pbf_block_header(entries, *td.name, range, 0);
		piece[i] = Piece{file, (size_t)(entries - file)};
	};
	if (nb >= 1024) {
		// many fonts in one group (21 fixture fonts: 2688 tasks per group, 2500 of them such files): 50 us on the calling
		// thread, which a run over many fonts has no device latency to hide behind — runs of 128 tasks on the pool
		constexpr size_t kRun = 128;
		pool().run((nb + kRun - 1) / kRun, [&](size_t c, unsigned) {
			for (size_t i = c * kRun; i < std::min(nb, (c + 1) * kRun); i++)
				if (G.task_g0[i] == G.task_g0[i + 1])
					empty_file(i);
		}, true);
		for (size_t i = 0; i < nb; i++)
			if (G.task_g0[i] != G.task_g0[i + 1])
				G.busy.push_back((uint32_t)i);
	} else {
		for (size_t i = 0; i < nb; i++) {
			if (G.task_g0[i] != G.task_g0[i + 1])
				G.busy.push_back((uint32_t)i);
			else
				empty_file(i);
		}
	}
	timings_.encode_s += now_s() - t3;
}

// A group submitted as ranges: the device has written every glyph's entry; what is left is the block header of every task, in
// the room in front of its first entry, from the tasks' extents.  The counters come from the rects
void FontManager::fe_assemble_ranges(const std::vector<Todo> &tasks, FeGroup &G)
{
	const double t3 = now_s();
	const FeGroup::Ranges &R = G.ranges;
	uint8_t *arena = G.out.data();
	for (const uint32_t i : G.busy) {
		const Todo &td = tasks[G.g0 + i];
		const uint32_t r0 = R.task_r0[i], r1 = R.task_r0[i + 1];
		if (r0 >= r1 || r1 >= R.extents.size() || R.extents[r1] > G.out_bytes || R.extents[r0] + R.pre[r0] > R.extents[r1])
			throw std::runtime_error("in-place PBF assembly: the device's extents of a task do not lie inside the arena");
		uint8_t *first = arena + R.extents[r0] + R.pre[r0], *end = arena + R.extents[r1];
		uint8_t *file = write_pbf_block_header(first, *td.name, td.block.range(), (size_t)(end - first));
		G.piece[i] = FeGroup::Piece{file, (size_t)(end - file)};
	}
	uint64_t n_raster = 0, n_pixels = 0;
	for (const vgsdf_rect &r : G.rects)
		if (r.has_raster) {
			n_raster++;
			n_pixels += (uint64_t)r.w * r.h;
		}
	G.n_raster = n_raster;
	G.n_pixels = n_pixels;
	timings_.encode_s += now_s() - t3;
}

void FontManager::fe_assemble(const std::vector<Todo> &tasks, FeGroup &G)
{
	if (G.by_ranges())
		return fe_assemble_ranges(tasks, G);
	ThreadPool &tp = pool();
	const double t3 = now_s();
	MergedOutlines &m = G.m;
	using Piece = FeGroup::Piece;
	std::vector<Piece> &piece = G.piece;
	std::atomic<uint64_t> n_raster{0}, n_pixels{0};
	std::atomic<bool> mismatch{false};
	uint8_t *arena = G.out.data();
	tp.run(G.busy.size(), [&](size_t bi, unsigned) {
		const size_t i = G.busy[bi];
		const Todo &td = tasks[G.g0 + i];
		const uint32_t a = G.task_g0[i], b = G.task_g0[i + 1];
		uint64_t rasters = 0, pixels = 0;
		uint8_t *first = nullptr, *end = nullptr;
		for (uint32_t g = a; g < b; g++) {
			const vgsdf_rect &r = G.rects[g];
			const GlyphJob &job = m.jobs[g];
			const bool has = r.has_raster != 0;
			// start of the entry from the bitmap's position: 0x1A varint(msg) 0x08 varint(id) [0x12 varint(w h)] come before it
			const uint64_t px = has ? (uint64_t)r.w * r.h : 0;
			const PbfEntrySize es = pbf_entry_size(job.id, job.advance, has, r.w, r.h, r.x0, r.y0);
			const uint64_t before = es.bitmap_at;
			if (G.pbf_at[g] < before || G.pbf_at[g] - before + es.total > G.out_bytes) {
				mismatch = true; // the entry does not lie inside the arena
				return;
			}
			uint8_t *entry = arena + (G.pbf_at[g] - before);
			if (g == a) {
				first = entry;
			} else if (entry != end) {
				mismatch = true; // the entries of a block follow each other without a gap
				return;
			}
			end = entry + write_pbf_entry_headers(entry, job.id, job.advance, has, r.w, r.h, r.x0, r.y0);
			rasters += has;
			pixels += px;
		}
		if ((size_t)(first - arena) < m.pbf_pre[a]) {
			mismatch = true;
			return;
		}
		uint8_t *file = write_pbf_block_header(first, *td.name, td.block.range(), (size_t)(end - first));
		piece[i] = Piece{file, (size_t)(end - file)};
		n_raster += rasters;
		n_pixels += pixels;
	}, true);
	if (mismatch)
		throw std::runtime_error("in-place PBF assembly: the device's layout of the arena differs from the host's");
	G.n_raster = n_raster;
	G.n_pixels = n_pixels;
	timings_.encode_s += now_s() - t3;
}

void FontManager::fe_write_pieces(const std::vector<Todo> &tasks, FeGroup &G, Writer &writer)
{
	const double t4 = now_s();
	const size_t nb = G.g1 - G.g0;
	std::string path;
	for (size_t i = 0; i < nb; i++) {
		tasks[G.g0 + i].block.path_into(*tasks[G.g0 + i].name, path);
		writer.write_bytes(path, G.piece[i].p, G.piece[i].n);
		timings_.pbf_bytes += G.piece[i].n;
	}
	timings_.write_s += now_s() - t4;
	timings_.blocks += nb;
	timings_.glyphs += G.n_jobs;
	timings_.rasters += G.n_raster;
	timings_.pixels += G.n_pixels;
	timings_.segments += G.n_segs;
}

// Rects + bitmaps of a rendered group -> PbfGlyphs per block (pool), written in task order.
void FontManager::fe_encode_write(const std::vector<Todo> &tasks, FeGroup &G, Writer &writer)
{
	ThreadPool &tp = pool();
	const double t3 = now_s();
	const size_t nb = G.g1 - G.g0;
	const uint32_t n_jobs = G.n_jobs;
	MergedOutlines &m = G.m;
	if (G.by_ranges()) { // no glyph was recorded: id and advance come from the families' host tables, range by range
		m.jobs.assign(n_jobs, GlyphJob{});
		const FeGroup::Ranges &R = G.ranges;
		uint32_t g = 0;
		for (size_t r = 0; r < R.first.size(); r++) {
			const FamilyTable &ft = *R.tables[R.family_of[r]];
			for (uint32_t e = R.entry_first[r]; e < ft.code_point.size() && ft.code_point[e] <= R.last[r] && g < n_jobs; e++, g++) {
				m.jobs[g].id = (ft.plane << 16) | ft.code_point[e];
				m.jobs[g].advance = ft.advance[e];
			}
		}
	}
	// bitmap offsets: rasterised glyphs are packed in job order
	std::vector<uint64_t> boff((size_t)n_jobs + 1, 0);
	uint64_t n_raster = 0;
	for (uint32_t g = 0; g < n_jobs; g++) {
		const vgsdf_rect &r = G.rects[g];
		GlyphJob &job = m.jobs[g];
		job.has_raster = r.has_raster != 0;
		job.x0 = r.x0;
		job.y0 = r.y0;
		job.width = r.w;
		job.height = r.h;
		job.x1 = r.x0 + (int32_t)r.w;
		job.y1 = r.y0 + (int32_t)r.h;
		job.n_segments = r.n_segments;
		boff[g + 1] = boff[g] + (job.has_raster ? (uint64_t)r.w * r.h : 0);
		n_raster += job.has_raster;
	}
	std::vector<std::pair<size_t, size_t>> span(nb, {0, 0});
	for (size_t i = 0; !G.by_ranges() && i < G.slices.size(); i++) {
		auto &sp = span[G.slices[i].task - G.g0];
		if (sp.second == 0)
			sp.first = i;
		sp.second = i + 1;
	}
	std::vector<std::vector<uint8_t>> encoded(nb);
	tp.run(nb, [&](size_t i, unsigned) {
		std::vector<PbfGlyphRef> refs;
		for (uint32_t g = G.by_ranges() ? G.task_g0[i] : 0; G.by_ranges() && g < G.task_g0[i + 1]; g++)
			refs.push_back(m.jobs[g].to_pbf(m.jobs[g].has_raster ? G.out.data() + boff[g] : nullptr));
		for (size_t k = span[i].first; k < span[i].second; k++) {
			const OSlice &s = G.slices[k];
			for (uint32_t j = 0; j < s.job1 - s.job0; j++) {
				const uint32_t g = s.g_job + j;
				const GlyphJob &job = m.jobs[g];
				refs.push_back(job.to_pbf(job.has_raster ? G.out.data() + boff[g] : nullptr));
			}
		}
		encoded[i] = PbfGlyphs::encode(*tasks[G.g0 + i].name, tasks[G.g0 + i].block.range(), std::move(refs));
	});
	const double t4 = now_s();
	timings_.encode_s += t4 - t3;
	for (size_t i = 0; i < nb; i++) {
		writer.write_file(*tasks[G.g0 + i].name + "/" + tasks[G.g0 + i].block.filename(), encoded[i]);
		timings_.pbf_bytes += encoded[i].size();
	}
	timings_.write_s += now_s() - t4;
	timings_.blocks += nb;
	timings_.glyphs += n_jobs;
	timings_.rasters += n_raster;
	timings_.pixels += G.out_bytes;
	timings_.segments += G.n_segs;
}

// Device front-end dispatcher: groups of tasks (part of a large font, or several small ones) go through
// record (host pool) -> device (flatten, raster; one submission, one synchronisation) -> encode + write (host
// pool).  Two groups are in flight: while the GPU works on group k the host records group k + 1 and then encodes
// group k - 1 (the submissions alternate between the renderer's two lanes = device contexts; the calling thread
// only enqueues and waits, there is no second host thread).  Files are written in task order; the first error
// aborts (manager.rs:117-121).
void FontManager::run_tasks_device_front_end(std::vector<Todo> &tasks, Writer &writer, const Renderer &renderer)
{
	timings_ = RenderTimings{};
	const double t_start = now_s();
	(void)pool();
	// Group size: every group costs ~0.1 ms of device latency and three fork/joins of the host pool, so small fonts
	// are grouped (21 fixture fonts: 12.9 ms one font per group, 2.1 ms in one group) and a run is cut into several
	// groups — to overlap host and device — only when each keeps >= 5000 glyphs (measured in round 3, 32 threads on a
	// 16-CPU quota: the 14 180 glyphs of the 21 fixture fonts 2.5 / 2.1 / 1.8 / 2.0 / 2.1 ms with groups of at least
	// 2000 / 3500 / 5000 / 8000 / 20 000 glyphs; Noto Sans' 6445 glyphs 1.14 / 1.09 / 1.07 ms at 2000 / 5000 / 20 000).
	// An explicit set_batch_blocks() bounds the group in blocks instead.  (Round 4: a half-size FIRST group, to start the device
	// earlier — 275 of the 21 fonts' 1110 us pass before the first submission — made three groups of two and the run slower,
	// 1106 -> 1271 us: with the host phases of a group at 120-220 us whatever its size the run is bound by this thread.)
	size_t total_glyphs = 0;
	for (const Todo &t : tasks)
		total_glyphs += t.block.len();
	constexpr size_t kFeGlyphBudget = 32768;
	static const char *mg = std::getenv("VG_FE_MIN_GROUP"); // (measurement switch)
	// (round 4, after the device stage and the host phases of a group got shorter: one or two fonts — up to 512 tasks — do best
	// in groups of >= 3000 glyphs: Noto Sans' 20 files, 6480 glyphs, 0.69 ms as one group, 0.60 ms as two, 0.79 ms as three;
	// a group's host cost grows with its TASKS, most of them empty blocks, so the 21 fixture fonts keep >= 5000: 1.05 ms in two
	// groups, 1.50 ms in four)
	const size_t kFeMinGroup = mg ? (size_t)std::max(1, std::atoi(mg)) : (tasks.size() <= 512 ? 3000 : 5000);
	const size_t n_groups = std::max<size_t>(1, total_glyphs / kFeMinGroup);
	const size_t budget = std::min(kFeGlyphBudget, (total_glyphs + n_groups - 1) / n_groups);
	std::vector<std::pair<size_t, size_t>> groups;
	for (size_t g0 = 0; g0 < tasks.size();) {
		size_t g1 = g0, glyphs = 0;
		while (g1 < tasks.size() && (batch_blocks_set_ ? g1 - g0 < (size_t)batch_blocks_ : (g1 == g0 || glyphs < budget))) {
			glyphs += tasks[g1].block.len();
			g1++;
		}
		groups.emplace_back(g0, g1);
		g0 = g1;
	}
	bool in_flight[2] = {false, false};
	// VG_TRACE_PHASES=1 (measurement switch): the calling thread's time line of the run, one line per group on stderr
	static const bool trace_ph = std::getenv("VG_TRACE_PHASES") != nullptr;
	struct Mark {
		const char *what;
		size_t k;
		double t;
	};
	std::vector<Mark> marks;
	auto mark = [&](const char *what, size_t k) {
		if (trace_ph)
			marks.push_back(Mark{what, k, now_s()});
	};
	auto submit = [&](size_t k) {
		FeGroup &G = fe_group_[k & 1];
		G.g0 = groups[k].first;
		G.g1 = groups[k].second;
		mark("record+pack >", k);
		fe_record(tasks, G, true, &renderer, (int)(k & 1));
		mark("submit >", k);
		const double t = now_s();
		if (G.n_jobs) {
			timings_.fe_groups++;
			timings_.fe_max_group_glyphs = std::max<uint64_t>(timings_.fe_max_group_glyphs, G.n_jobs);
			uint64_t block = 0;
			switch (G.form) { // the view the renderer is handed, and the counters the group raises
			case GroupForm::RangesGlyf:
			case GroupForm::RangesCommands: // (counted as family groups and not among the named ones)
				renderer.submit_ranges((int)(k & 1), G.ranges.view(G.in_place), G.n_jobs, G.out, &block);
				timings_.family_groups++;
				timings_.family_block_bytes += block;
				break;
			case GroupForm::NamedGlyf:
				renderer.submit_outlines((int)(k & 1), G.m.view_resident(), G.out, &block);
				timings_.resident_groups++;
				timings_.resident_block_bytes += block;
				break;
			case GroupForm::NamedCommands:
				renderer.submit_outlines((int)(k & 1), G.m.view_resident(), G.out, &block);
				timings_.command_groups++;
				timings_.command_block_bytes += block;
				break;
			case GroupForm::RangesMixed: // (counted as mixed groups, and among no others)
			case GroupForm::NamedMixed:
				if (G.form == GroupForm::RangesMixed)
					renderer.submit_ranges((int)(k & 1), G.ranges.view(G.in_place), G.n_jobs, G.out, &block);
				else
					renderer.submit_outlines((int)(k & 1), G.m.view_resident(), G.out, &block, true);
				timings_.mixed_groups++;
				timings_.mixed_glyf_fonts += G.mixed_glyf_stores;
				timings_.mixed_command_fonts += G.mixed_command_stores;
				timings_.mixed_block_bytes += block;
				break;
			case GroupForm::GlyfParts:
				renderer.submit_outlines((int)(k & 1), G.m.view_glyf(), G.out);
				timings_.glyf_groups++;
				break;
			case GroupForm::Packed:
				renderer.submit_outlines((int)(k & 1), G.m.view(), G.out);
				break;
			}
			in_flight[k & 1] = true;
		}
		timings_.device_s += now_s() - t;
		mark("submitted", k);
	};
	auto collect = [&](size_t k) {
		FeGroup &G = fe_group_[k & 1];
		double t = now_s();
		mark("pieces >", k);
		G.rects.clear();
		G.out_bytes = G.n_segs = 0;
		// in-place assembly: the rects come back right behind the plan kernel, a good 100 us before the bitmaps — the
		// headers are written while the raster is still storing the bitmaps between them
		bool early = false;
		if (G.in_place && G.n_jobs)
			fe_prepare_pieces(tasks, G);
		t = now_s();
		mark("peek >", k);
		if (in_flight[k & 1] && G.in_place && G.n_jobs) {
			early = renderer.peek_outlines((int)(k & 1), G.rects, G.out_bytes, G.n_jobs, &G.pbf_at);
			timings_.device_s += now_s() - t;
			mark("assemble >", k);
			if (early && G.by_ranges())
				renderer.task_extents((int)(k & 1), G.ranges.extents, (uint32_t)G.ranges.first.size());
			if (early)
				fe_assemble(tasks, G);
			t = now_s();
		}
		mark("wait >", k);
		if (in_flight[k & 1]) {
			in_flight[k & 1] = false;
			try {
				renderer.wait_outlines((int)(k & 1), G.rects, G.out, G.out_bytes, G.n_segs, G.n_jobs, G.in_place ? &G.pbf_at : nullptr);
			} catch (const GlyfEntryError &) {
				// a malformed `glyf` entry somewhere in the group: ttf-parser's rules for such glyphs (None for the glyph, the
				// rest of a composite skipped) are the host reader's — the group is recorded there and rendered again, now
				early = false;
				timings_.glyf_fallbacks++;
				for (size_t tk = G.g0; tk < G.g1; tk++) // (later groups and runs of these fonts skip the glyf form)
					glyf_refused_.insert(tasks[tk].name);
				const std::vector<uint32_t> g0_before = G.task_g0;
				fe_record(tasks, G, false);
				// the pieces prepared above (files of the empty blocks, list of the others) depend on which jobs a task has: both
				// recorders must look up the same glyphs
				if (G.task_g0 != g0_before)
					throw std::runtime_error("render_glyphs: the host's reader and the glyf parts disagree on a group's glyphs");
				t = now_s();
				renderer.submit_outlines((int)(k & 1), G.m.view(), G.out);
				renderer.wait_outlines((int)(k & 1), G.rects, G.out, G.out_bytes, G.n_segs, G.n_jobs, G.in_place ? &G.pbf_at : nullptr);
			}
		}
		timings_.device_s += now_s() - t;
		mark("write >", k);
		if (G.in_place && G.n_jobs) {
			if (!early && G.by_ranges())
				renderer.task_extents((int)(k & 1), G.ranges.extents, (uint32_t)G.ranges.first.size());
			if (!early)
				fe_assemble(tasks, G);
			fe_write_pieces(tasks, G, writer);
		} else {
			fe_encode_write(tasks, G, writer);
		}
		mark("done", k);
	};
	try {
		for (size_t k = 0; k < groups.size(); k++) {
			submit(k);
			if (k > 0)
				collect(k - 1);
		}
		if (!groups.empty())
			collect(groups.size() - 1);
	} catch (...) {
		// leave no submission behind (its lane stays held until it is waited for)
		for (int lane = 0; lane < 2; lane++)
			if (in_flight[lane]) {
				in_flight[lane] = false;
				try {
					FeGroup &G = fe_group_[lane];
					renderer.wait_outlines(lane, G.rects, G.out, G.out_bytes, G.n_segs, G.n_jobs);
				} catch (...) {
				}
			}
		throw;
	}
	timings_.total_s = now_s() - t_start;
	if (trace_ph) {
		std::string line = "[phases] " + std::to_string(groups.size()) + " groups, " + std::to_string(total_glyphs) + " glyphs:";
		char buf[96];
		for (const Mark &mk : marks) {
			std::snprintf(buf, sizeof buf, " | %s g%zu @%.0f", mk.what, mk.k, (mk.t - t_start) * 1e6);
			line += buf;
		}
		std::snprintf(buf, sizeof buf, " | end @%.0f us\n", timings_.total_s * 1e6);
		line += buf;
		std::fputs(line.c_str(), stderr);
	}
}

} // namespace vg
