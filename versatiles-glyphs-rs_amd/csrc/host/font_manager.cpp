#include "font_manager.hpp"

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <thread>

#include "font_manager_internal.hpp"
#include "index_files.hpp"

namespace vg {

namespace {

bool read_file(const std::string &path, std::vector<uint8_t> &out, std::string *err)
{
	std::ifstream f(path, std::ios::binary | std::ios::ate);
	if (!f) {
		if (err)
			*err = "reading font file \"" + path + "\""; // wrapper.rs:35 context string
		return false;
	}
	const std::streamsize n = f.tellg();
	f.seekg(0);
	out.resize((size_t)n);
	if (n && !f.read((char *)out.data(), n)) {
		if (err)
			*err = "reading font file \"" + path + "\"";
		return false;
	}
	return true;
}

} // namespace

// manager.rs:141-147: lower-case, runs of [-_\s] -> one separator, trim, ' ' -> '_'
std::string name_to_id(const std::string &name)
{
	std::string out;
	bool pending_sep = false;
	for (unsigned char c : name) {
		const bool sep = c == '-' || c == '_' || c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v';
		if (sep) {
			pending_sep = !out.empty();
			continue;
		}
		if (pending_sep) {
			out.push_back('_');
			pending_sep = false;
		}
		out.push_back((c >= 'A' && c <= 'Z') ? (char)(c - 'A' + 'a') : (char)c);
	}
	return out;
}

std::unique_ptr<FontFileEntry> FontFileEntry::create(std::vector<uint8_t> data, std::string *err, const std::vector<int16_t> *coords, bool gvar_advances)
{
	return create(std::make_shared<const std::vector<uint8_t>>(std::move(data)), err, coords, nullptr, gvar_advances);
}

std::unique_ptr<FontFileEntry> FontFileEntry::create(std::shared_ptr<const std::vector<uint8_t>> data, std::string *err,
                                                     const std::vector<int16_t> *coords, const std::string *ps_name, bool gvar_advances)
{
	std::unique_ptr<FontFileEntry> e(new FontFileEntry());
	e->data_ = std::move(data);
	std::string why = "font parse failed";
	auto face = coords ? Face::parse_at(e->data_->data(), e->data_->size(), *coords, &why, gvar_advances) : Face::parse(e->data_->data(), e->data_->size());
	if (!face) {
		if (err)
			*err = why;
		return nullptr;
	}
	e->face_ = *face;
	if (!e->face_.has_cmap()) { // metadata.rs:104-107
		if (err)
			*err = "Font has no cmap table";
		return nullptr;
	}
	// The reference renders `glyf`, `CFF ` and `CFF2` outlines through ttf-parser, and so does this reader.  A font
	// whose only outline table it cannot open (a malformed `CFF ` / `CFF2`: the crate drops such a table and renders
	// empty glyphs) is refused loudly instead of writing PBFs whose glyphs are all empty.  (A font with no outline
	// table at all renders empty glyphs in the reference too: outline_glyph -> None.)
	if (e->face_.has_unsupported_outlines()) {
		if (err)
			*err = "the font's CFF / CFF2 table cannot be read and it has no glyf outlines";
		return nullptr;
	}
	e->codepoints_ = e->face_.unicode_codepoints();
	{
		// metadata.rs:92-103: HashMap::from_iter over the name records — a later record of the same id
		// replaces an earlier one, and a record ttf-parser cannot decode counts as an empty string
		std::map<uint16_t, std::string> names;
		for (auto &kv : e->face_.names())
			names[kv.first] = std::move(kv.second);
		e->metadata_.name = names.count(1) ? names[1] : std::string(); // name_id::FAMILY
		const ParsedFontName pn = parse_font_name(e->metadata_.name, ps_name ? *ps_name : names.count(6) ? names[6] : std::string()); // POST_SCRIPT_NAME
		e->metadata_.family = pn.family;
		e->metadata_.style = pn.style;
		e->metadata_.weight = pn.weight;
		e->metadata_.width = pn.width;
	}
	return e;
}

const std::string &GlyphBlock::range() const
{
	// "{start}-{start + 255}" (glyph_block.rs:53-59); start is a multiple of 256 below 65536 (wrapper.rs:55-60)
	static const std::vector<std::string> table = [] {
		std::vector<std::string> t;
		for (uint32_t s = 0; s < 0x10000; s += GLYPH_BLOCK_SIZE)
			t.push_back(std::to_string(s) + "-" + std::to_string(s + GLYPH_BLOCK_SIZE - 1));
		return t;
	}();
	static thread_local std::string other;
	if (start_index % GLYPH_BLOCK_SIZE == 0 && start_index < 0x10000)
		return table[start_index / GLYPH_BLOCK_SIZE];
	other = std::to_string(start_index) + "-" + std::to_string(start_index + GLYPH_BLOCK_SIZE - 1);
	return other;
}

void GlyphBlock::prepare(TessScratch &scratch, GlyphBatch &batch, uint32_t ci0, uint32_t ci1) const
{
	for (uint32_t ci = ci0; ci < ci1 && ci < GLYPH_BLOCK_SIZE; ci++)
		if (const FontFileEntry *f = glyphs[ci])
			Renderer::prepare(f->face(), start_index + ci, scratch, batch);
}

std::vector<uint8_t> GlyphBlock::render(const std::string &font_name, const Renderer &renderer) const
{
	TessScratch scratch;
	GlyphBatch batch;
	prepare(scratch, batch);
	std::vector<uint8_t> pixels((size_t)batch.out_bytes());
	renderer.render_batch(batch, pixels.data());
	std::vector<PbfGlyphRef> refs;
	refs.reserve(batch.jobs.size());
	size_t r = 0;
	for (const GlyphJob &j : batch.jobs) {
		const uint8_t *bm = j.has_raster ? pixels.data() + batch.out_off[r++] : nullptr;
		refs.push_back(j.to_pbf(bm));
	}
	return PbfGlyphs::encode(font_name, range(), std::move(refs));
}

bool FontWrapper::add_paths(const std::vector<std::string> &paths, std::string *err)
{
	for (const std::string &p : paths) {
		std::vector<uint8_t> data;
		if (!read_file(p, data, err))
			return false;
		auto e = FontFileEntry::create(std::move(data), err);
		if (!e)
			return false;
		files_.push_back(std::move(e));
		blocks_valid_ = false;
	}
	return true;
}

std::vector<GlyphBlock> FontWrapper::get_blocks() const
{
	std::vector<GlyphBlock> blocks(kBmpBlocks);
	for (uint32_t i = 0; i < kBmpBlocks; i++)
		blocks[i].start_index = i * GLYPH_BLOCK_SIZE;
	std::map<uint32_t, GlyphBlock> above; // by start, populated ones only
	for (const auto &file : files_)
		for (uint32_t cp : file->codepoints()) {
			if (cp > 0xFFFF) { // wrapper.rs:66-68, unless the supplementary planes are on
				if (!supplementary_ || cp > 0x10FFFF)
					continue;
				GlyphBlock &b = above[cp / GLYPH_BLOCK_SIZE * GLYPH_BLOCK_SIZE];
				b.start_index = cp / GLYPH_BLOCK_SIZE * GLYPH_BLOCK_SIZE;
				b.set_glyph_font((uint8_t)(cp % GLYPH_BLOCK_SIZE), file.get());
				continue;
			}
			blocks[cp / GLYPH_BLOCK_SIZE].set_glyph_font((uint8_t)(cp % GLYPH_BLOCK_SIZE), file.get());
		}
	for (auto &kv : above)
		blocks.push_back(std::move(kv.second));
	return blocks;
}

const GlyphBlock *FontWrapper::find_block(const std::vector<GlyphBlock> &blocks, uint32_t start)
{
	if (start % GLYPH_BLOCK_SIZE)
		return nullptr;
	if (start < 0x10000)
		return start / GLYPH_BLOCK_SIZE < blocks.size() ? &blocks[start / GLYPH_BLOCK_SIZE] : nullptr;
	const auto first = blocks.begin() + std::min<size_t>(kBmpBlocks, blocks.size());
	const auto it = std::lower_bound(first, blocks.end(), start, [](const GlyphBlock &b, uint32_t s) { return b.start_index < s; });
	return it != blocks.end() && it->start_index == start ? &*it : nullptr;
}

FontManager::~FontManager() = default;

FontManager::FontManager(const FontManager *parent, uint32_t rank, uint32_t world)
    : parent_(parent), parallel_(parent->parallel_)
{
	shard_rank_ = rank;
	shard_world_ = world;
	device_front_end_ = parent->device_front_end_;
	batch_blocks_ = parent->batch_blocks_;
	batch_blocks_set_ = parent->batch_blocks_set_;
}

// a font changed: shard tables, the ranks' filtered block tables and the lanes that hold them are stale
void FontManager::invalidate_shards()
{
	std::lock_guard<std::mutex> lock(shard_mu_);
	shard_cache_.clear();
	shard_blocks_.clear();
	children_.clear();
	lane_plan_ = LanePlan{};
	glyf_refused_.clear();
}

FontWrapper &FontManager::font_slot(const std::string &font_id)
{
	FontWrapper &w = fonts_[font_id];
	w.set_supplementary(supplementary_planes_);
	return w;
}

void FontManager::set_supplementary_planes(bool on)
{
	if (on == supplementary_planes_)
		return;
	supplementary_planes_ = on;
	invalidate_shards(); // (the lane plan and the ranks' tables point into the block tables rebuilt below)
	for (auto &kv : fonts_)
		kv.second.set_supplementary(on);
}

bool FontManager::add_font_with_name(const std::string &name, const std::vector<std::string> &sources, std::string *err)
{
	invalidate_shards();
	return font_slot(name_to_id(name)).add_paths(sources, err);
}

bool FontManager::add_font_data(const std::string &name, std::vector<uint8_t> data, std::string *err)
{
	auto e = FontFileEntry::create(std::move(data), err);
	if (!e)
		return false;
	invalidate_shards();
	font_slot(name_to_id(name)).add_file(std::move(e));
	return true;
}

bool FontManager::add_font_instance_normalized(const std::string &name, std::vector<uint8_t> data, const std::vector<int16_t> &coords,
                                               std::string *err)
{
	auto e = FontFileEntry::create(std::move(data), err, &coords, gvar_advances_);
	if (!e)
		return false;
	gvar_advance_faces_ += e->face().advances_by_gvar();
	invalidate_shards();
	font_slot(name_to_id(name)).add_file(std::move(e));
	return true;
}

bool FontManager::add_font_instance(const std::string &name, std::vector<uint8_t> data, const std::vector<std::array<char, 4>> &tags,
                                    const std::vector<float> &values, std::string *err)
{
	auto refuse = [&](const std::string &why) {
		if (err)
			*err = why;
		return false;
	};
	std::vector<VariationAxis> axes;
	if (!read_variation_axes(data.data(), data.size(), axes))
		return refuse("a position needs a readable fvar table, and this file has none");
	if (tags.size() != values.size())
		return refuse("add_font_instance: as many values as tags");
	if (axes.size() > 64)
		axes.resize(64); // (the face counts no more)
	std::vector<int16_t> coords(axes.size(), 0);
	std::vector<bool> given(axes.size(), false);
	for (size_t k = 0; k < tags.size(); k++) {
		const std::string tag(tags[k].data(), 4);
		if (!std::isfinite(values[k]))
			return refuse("axis " + tag + ": a value that is not finite");
		size_t i = 0;
		while (i < axes.size() && std::memcmp(axes[i].tag, tags[k].data(), 4) != 0)
			i++;
		if (i == axes.size())
			return refuse("axis " + tag + ": the file's fvar has no such axis");
		if (given[i])
			return refuse("axis " + tag + ": given twice");
		given[i] = true;
		coords[i] = normalize_axis_value(axes[i], values[k]);
	}
	apply_avar(data.data(), data.size(), coords);
	return add_font_instance_normalized(name, std::move(data), coords, err);
}

bool FontManager::add_font_named_instances(std::vector<uint8_t> data, std::vector<std::string> &ids, std::string *err)
{
	auto refuse = [&](const std::string &why) {
		if (err)
			*err = why;
		return false;
	};
	std::vector<VariationAxis> axes;
	std::vector<NamedInstance> instances;
	if (!read_variation_axes(data.data(), data.size(), axes, &instances))
		return refuse("named instances need a readable fvar table, and this file has none");
	if (instances.empty())
		return refuse("the file's fvar has no instance record");
	std::string family;
	std::vector<std::string> ps_names;
	if (!named_instance_ps_names(data.data(), data.size(), instances, family, ps_names))
		return refuse("font parse failed");
	if (axes.size() > 64)
		axes.resize(64); // (the face counts no more)
	const auto bytes = std::make_shared<const std::vector<uint8_t>>(std::move(data));
	std::vector<std::unique_ptr<FontFileEntry>> entries;
	for (size_t k = 0; k < instances.size(); k++) {
		std::vector<int16_t> coords(axes.size(), 0);
		for (size_t i = 0; i < axes.size(); i++)
			coords[i] = normalize_axis_value(axes[i], instances[k].coords[i]);
		apply_avar(bytes->data(), bytes->size(), coords);
		auto e = FontFileEntry::create(bytes, err, &coords, &ps_names[k], gvar_advances_);
		if (!e)
			return false;
		entries.push_back(std::move(e));
	}
	invalidate_shards();
	ids.clear();
	InstanceGroup &group = instance_groups_[bytes->data()];
	for (auto &e : entries) {
		gvar_advance_faces_ += e->face().advances_by_gvar();
		ids.push_back(name_to_id(e->metadata().generate_name()));
		group.faces.push_back(&e->face()), group.ids.push_back(ids.back());
		instance_bytes_of_[&e->face()] = bytes->data();
		font_slot(ids.back()).add_file(std::move(e));
	}
	return true;
}

const FontManager::InstanceGroup *FontManager::instance_group_of(const Face &face) const
{
	const FontManager &root = parent_ ? *parent_ : *this;
	const auto key = root.instance_bytes_of_.find(&face);
	if (key == root.instance_bytes_of_.end())
		return nullptr;
	const auto group = root.instance_groups_.find(key->second);
	return group == root.instance_groups_.end() ? nullptr : &group->second;
}

std::vector<std::string> FontManager::instance_group(const std::string &font_id) const
{
	const auto it = fonts().find(font_id);
	if (it == fonts().end() || it->second.files().size() != 1)
		return {};
	const InstanceGroup *group = instance_group_of(it->second.files()[0]->face());
	return group ? group->ids : std::vector<std::string>{};
}

bool FontManager::charstring2_group(const std::string &font_id, Charstring2Group &out, std::string *err) const
{
	if (!charstring2_table(font_id, 0, err))
		return false;
	const auto it = fonts().find(font_id);
	const InstanceGroup *group = it == fonts().end() || it->second.files().size() != 1 ? nullptr : instance_group_of(it->second.files()[0]->face());
	if (!group) {
		if (err)
			*err = "font '" + font_id + "': not one file of an instance group";
		return false;
	}
	std::call_once(group->charstring2_once, [&] {
		const CharstringTable &first = group->faces[0]->charstring2_table();
		std::vector<float> all;
		for (const Face *f : group->faces) {
			const CharstringTable &t = f->charstring2_table();
			if (!t.ok || !first.ok || !t.same_face(first))
				return;
			all.insert(all.end(), t.factors.begin(), t.factors.end());
		}
		group->charstring2_factors.swap(all);
		group->charstring2_alike = true;
	});
	if (!group->charstring2_alike) {
		if (err)
			*err = "font '" + font_id + "': the faces of its instance group have no `CFF2` charstrings in common";
		return false;
	}
	out.first = &group->faces[0]->charstring2_table();
	out.factors = group->charstring2_factors.data();
	out.n_positions = (uint32_t)group->faces.size();
	return true;
}

bool FontManager::add_path(const std::string &path, std::string *err)
{
	std::vector<uint8_t> data;
	if (!read_file(path, data, err))
		return false;
	if (scan_named_instances_) {
		std::vector<VariationAxis> axes;
		std::vector<NamedInstance> instances;
		if (read_variation_axes(data.data(), data.size(), axes, &instances) && !instances.empty()) {
			std::vector<std::string> ids;
			return add_font_named_instances(std::move(data), ids, err);
		}
	}
	auto e = FontFileEntry::create(std::move(data), err);
	if (!e)
		return false;
	invalidate_shards();
	font_slot(name_to_id(e->metadata().generate_name())).add_file(std::move(e));
	return true;
}

bool FontManager::add_paths(const std::vector<std::string> &paths, std::string *err)
{
	for (const std::string &p : paths)
		if (!add_path(p, err))
			return false;
	return true;
}

bool FontManager::scan(const std::string &path, std::string *err)
{
	struct stat st;
	if (::stat(path.c_str(), &st) != 0) // is_file() / is_dir() are both false: nothing to do (recurse.rs:105-111)
		return true;
	if (S_ISREG(st.st_mode)) {
		// Path::extension(): what follows the last '.' of the file name (none for ".ttf" itself)
		const size_t slash = path.find_last_of('/');
		const std::string fname = slash == std::string::npos ? path : path.substr(slash + 1);
		const size_t dot = fname.find_last_of('.');
		const std::string ext = (dot == std::string::npos || dot == 0) ? std::string() : fname.substr(dot + 1);
		if (ext == "ttf" || ext == "otf")
			return add_path(path, err);
		return true;
	}
	if (!S_ISDIR(st.st_mode))
		return true;
	const std::string base = (!path.empty() && path.back() == '/') ? path : path + "/";
	const std::string cfg = base + "fonts.json";
	if (::stat(cfg.c_str(), &st) == 0) {
		std::vector<uint8_t> data;
		if (!read_file(cfg, data, err)) {
			if (err)
				*err = "Failed to read \"" + cfg + "\": " + *err;
			return false;
		}
		std::vector<FontConfig> configs;
		if (!parse_fonts_json(std::string(data.begin(), data.end()), configs, err))
			return false;
		for (const FontConfig &c : configs) {
			std::vector<std::string> sources;
			for (const std::string &src : c.sources)
				sources.push_back((!src.empty() && src[0] == '/') ? src : base + src); // Path::join
			if (!add_font_with_name(c.name, sources, err))
				return false;
		}
		return true;
	}
	DIR *d = ::opendir(path.c_str());
	if (!d) {
		if (err)
			*err = "reading directory \"" + path + "\": " + std::strerror(errno);
		return false;
	}
	std::vector<std::string> names;
	while (struct dirent *ent = ::readdir(d)) {
		const std::string n = ent->d_name;
		if (n != "." && n != "..")
			names.push_back(n);
	}
	::closedir(d);
	std::sort(names.begin(), names.end());
	for (const std::string &n : names)
		if (!scan(base + n, err))
			return false;
	return true;
}

void FontManager::write_index_json(Writer &writer) const { writer.write_file("index.json", build_index_json(*this)); }

void FontManager::write_families_json(Writer &writer) const
{
	writer.write_file("font_families.json", build_font_families_json(*this));
}

// CPUs this process may actually run on at once: the cgroup's CPU quota when there is one (containers: cpu.max =
// "quota period"), else the scheduler affinity / hardware_concurrency.
static unsigned cpu_budget()
{
	unsigned n = std::thread::hardware_concurrency();
	if (std::FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
		char q[32] = {0};
		long long period = 0;
		if (std::fscanf(f, "%31s %lld", q, &period) == 2 && period > 0 && std::strcmp(q, "max") != 0) {
			const long long quota = std::atoll(q);
			if (quota > 0)
				n = (unsigned)std::min<long long>(n ? n : 1u << 20, (quota + period - 1) / period);
		}
		std::fclose(f);
	}
	return n ? n : 1;
}

unsigned FontManager::worker_count() const
{
	if (!parallel_)
		return 1;
	if (threads_)
		return threads_;
	// VG_THREADS or set_threads() override.  Default: 1.5 x the CPUs the process may use, at most 64 (beyond that the
	// fork / join of a phase costs more than the phase; rounds 1-2 capped the pool at 16).  The phases are a few hundred
	// microseconds long and some threads beyond one per CPU hide the wake-up of the others — but a container's CPU quota
	// counts CPU TIME per 100 ms period, spinning included, and a run longer than one period is throttled when pool +
	// spinners exceed it (tools/sustained_e2e.py on a 16-CPU quota, 2 s runs, glyphs/s of the 21 fixture fonts / of Noto
	// Sans Regular alone: 32 threads that all spin 100 us after a fork 5.0-5.6 M / 3.2-3.6 M with 29 of 30 periods
	// throttled — the setting round 3 first chose from runs of a few milliseconds, where it is the fastest —; 32 threads,
	// no spinning 7.1-8.1 / 4.4-5.2; 16 threads, all spinning 5.9-7.1 / 5.2-5.8; 24 threads of which at most 2 spin
	// 8.4 / 6.0, nothing throttled).  The spinner limit is the pool's (thread_pool.hpp).
	if (const char *e = std::getenv("VG_THREADS"))
		if (int v = std::atoi(e); v > 0)
			return (unsigned)v;
	static const unsigned budget = cpu_budget();
	return std::max(1u, std::min(budget + budget / 2, 64u));
}

ThreadPool &FontManager::pool()
{
	const unsigned want = worker_count();
	if (!pool_ || pool_->size() != want) {
		pool_.reset(new ThreadPool(want));
		workers_.clear();
		workers_.resize(want);
	}
	return *pool_;
}

void FontManager::tessellate_and_pack(const std::vector<Todo> &tasks, size_t t0, size_t t1,
                                      std::vector<Slice> &slices, PackedBatch &out)
{
	constexpr uint32_t kSlice = 64; // code points per unit of host work
	ThreadPool &tp = pool();
	slices.clear();
	for (size_t t = t0; t < t1; t++) {
		if (tasks[t].block.is_empty())
			continue;
		for (uint32_t c = 0; c < GLYPH_BLOCK_SIZE; c += kSlice) {
			Slice s;
			s.task = (uint32_t)t;
			s.ci0 = c;
			s.ci1 = c + kSlice;
			slices.push_back(s);
		}
	}
	for (Worker &w : workers_)
		w.local.clear();
	const double t_begin = now_s();

	// T: tessellate every slice into its worker's local batch (capacity is retained run to run)
	tp.run(slices.size(), [&](size_t i, unsigned wid) {
		Slice &s = slices[i];
		Worker &w = workers_[wid];
		s.worker = wid;
		s.job0 = (uint32_t)w.local.jobs.size();
		s.raster0 = (uint32_t)w.local.n_raster();
		tasks[s.task].block.prepare(w.scratch, w.local, s.ci0, s.ci1);
		s.job1 = (uint32_t)w.local.jobs.size();
		s.raster1 = (uint32_t)w.local.n_raster();
	});

	const double t_tess_done = now_s();
	// P: positions in the packed batch, in task order (deterministic: ascending id per font)
	uint32_t rasters = 0;
	uint64_t segs = 0, pixels = 0;
	for (Slice &s : slices) {
		const GlyphBatch &l = workers_[s.worker].local;
		s.g_raster = rasters;
		s.g_seg = segs;
		s.g_out = pixels;
		rasters += s.raster1 - s.raster0;
		segs += l.seg_off[s.raster1] - l.seg_off[s.raster0];
		pixels += l.out_off[s.raster1] - l.out_off[s.raster0];
	}
	if (segs > 0xFFFFFFFFull)
		throw std::runtime_error("batch exceeds 2^32 segments; lower set_batch_blocks()");
	out.reserve(rasters, segs, pixels);
	out.n_raster = rasters;
	out.n_seg = segs;
	out.out_bytes = pixels;

	// C: copy the slices into the page-locked SoA arrays
	tp.run(slices.size(), [&](size_t i, unsigned) {
		const Slice &s = slices[i];
		const GlyphBatch &l = workers_[s.worker].local;
		const uint32_t ls0 = l.seg_off[s.raster0];
		const size_t n = l.seg_off[s.raster1] - ls0;
		if (n) {
			std::memcpy(out.sx.data() + s.g_seg, l.sx.data() + ls0, n * sizeof(double));
			std::memcpy(out.sy.data() + s.g_seg, l.sy.data() + ls0, n * sizeof(double));
			std::memcpy(out.ex.data() + s.g_seg, l.ex.data() + ls0, n * sizeof(double));
			std::memcpy(out.ey.data() + s.g_seg, l.ey.data() + ls0, n * sizeof(double));
		}
		const uint64_t lo0 = l.out_off[s.raster0];
		for (uint32_t r = s.raster0; r < s.raster1; r++) {
			const uint32_t g = s.g_raster + (r - s.raster0);
			out.x0[g] = l.x0[r];
			out.y0[g] = l.y0[r];
			out.w[g] = l.w[r];
			out.h[g] = l.h[r];
			out.seg_off[g + 1] = (uint32_t)(s.g_seg + (l.seg_off[r + 1] - ls0));
			out.out_off[g + 1] = s.g_out + (l.out_off[r + 1] - lo0);
		}
	});
	timings_.tessellate_s += t_tess_done - t_begin;
	timings_.pack_s += now_s() - t_tess_done;
}

const FontManager::FontEntry *FontManager::find_font(const std::string &font_id, std::string *err) const
{
	auto it = fonts().find(font_id);
	if (it != fonts().end())
		return &*it;
	if (err)
		*err = "unknown font id " + font_id;
	return nullptr;
}

bool FontManager::build_batch(const std::string &font_id, PackedBatch &out, std::vector<uint32_t> &ids,
                              uint32_t &n_jobs, std::string *err)
{
	const FontEntry *it = find_font(font_id, err);
	if (!it)
		return false;
	std::vector<Todo> tasks;
	for (const GlyphBlock &b : task_blocks(it->first, it->second))
		tasks.push_back(Todo{&it->first, b});
	std::vector<Slice> slices;
	tessellate_and_pack(tasks, 0, tasks.size(), slices, out);
	ids.assign(out.n_raster, 0);
	n_jobs = 0;
	for (const Slice &s : slices) {
		const GlyphBatch &l = workers_[s.worker].local;
		n_jobs += s.job1 - s.job0;
		for (uint32_t r = s.raster0; r < s.raster1; r++)
			ids[s.g_raster + (r - s.raster0)] = l.jobs[l.raster_job[r]].id;
	}
	return true;
}

bool FontManager::record_outlines(const std::string &font_id, OutlineBatch &out, std::string *err) const
{
	const FontEntry *it = find_font(font_id, err);
	if (!it)
		return false;
	out.clear();
	for (const GlyphBlock &b : task_blocks(it->first, it->second))
		for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE; ci++)
			if (const FontFileEntry *f = b.glyphs[ci])
				Renderer::record(f->face(), b.start_index + ci, out);
	return true;
}

bool FontManager::record_glyf_parts(const std::string &font_id, GlyfPartsBatch &out, std::string *err) const
{
	const FontEntry *it = find_font(font_id, err);
	if (!it)
		return false;
	out.clear();
	for (const GlyphBlock &b : task_blocks(it->first, it->second)) {
		if (!b.all_glyf) {
			if (err)
				*err = "font " + font_id + " has glyphs without glyf outlines (CFF / CFF2): the device decodes glyf entries only";
			return false;
		}
		for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE; ci++)
			if (const FontFileEntry *f = b.glyphs[ci])
				Renderer::record_parts(f->face(), b.start_index + ci, out);
		if (out.overflow) {
			if (err)
				*err = "font " + font_id + ": the glyf parts of a glyph pass the batch bounds (composite fan-out): not a batch for the device's decoder";
			return false;
		}
	}
	return true;
}

bool FontManager::record_named(const std::string &font_id, ResidentBatch &out, bool commands, std::string *err) const
{
	const FontEntry *it = find_font(font_id, err);
	if (!it)
		return false;
	out.clear();
	const auto &files = it->second.files();
	std::map<const FontFileEntry *, uint16_t> file_of;
	for (size_t k = 0; k < files.size(); k++) {
		const Face &face = files[k]->face();
		if (k > 0xFFFF || !(commands ? face.command_table().ok : face.resident_table().ok)) {
			if (err)
				*err = "font " + font_id + (commands ? ": a file whose outline commands pass what 32-bit offsets address"
				                                     : ": a file without `glyf` outlines, or past the bounds of the resident form (composite fan-out)");
			return false;
		}
		file_of.emplace(files[k].get(), (uint16_t)k);
	}
	for (const GlyphBlock &b : task_blocks(it->first, it->second))
		for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE; ci++)
			if (const FontFileEntry *f = b.glyphs[ci])
				Renderer::record_resident(f->face(), file_of.at(f), b.start_index + ci, out);
	return true;
}

// one of a file's outline tables by (font id, file index); `why`: what a table that is not ok means
template <class Table>
const Table *FontManager::file_table(const std::string &font_id, size_t file_index, const Table &(Face::*table)() const, const char *why,
                                     std::string *err) const
{
	auto it = fonts().find(font_id);
	if (it == fonts().end() || file_index >= it->second.files().size()) {
		if (err)
			*err = "unknown font id " + font_id + ", or a file index past its files";
		return nullptr;
	}
	const Table &t = (it->second.files()[file_index]->face().*table)();
	if (!t.ok) {
		if (err)
			*err = "font " + font_id + ": " + why;
		return nullptr;
	}
	return &t;
}

const ResidentTable *FontManager::resident_table(const std::string &font_id, size_t file_index, std::string *err) const
{
	return file_table(font_id, file_index, &Face::resident_table,
	                  "the file has no `glyf` outlines, or is past the bounds of the resident form (composite fan-out)", err);
}

const CommandTable *FontManager::command_table(const std::string &font_id, size_t file_index, std::string *err) const
{
	return file_table(font_id, file_index, &Face::command_table, "the file's outline commands pass what 32-bit offsets address", err);
}

const CharstringTable *FontManager::charstring_table(const std::string &font_id, size_t file_index, std::string *err) const
{
	return file_table(font_id, file_index, &Face::charstring_table,
	                  "the file has no `CFF ` version 1 charstrings the device's decoder could be given", err);
}

const CharstringTable *FontManager::charstring2_table(const std::string &font_id, size_t file_index, std::string *err) const
{
	return file_table(font_id, file_index, &Face::charstring2_table, "the file has no `CFF2` charstrings the device's decoder could be given", err);
}

namespace {
uint64_t next_family_serial()
{
	static std::atomic<uint64_t> next_serial{1};
	return next_serial++;
}
} // namespace

FontManager::FamilyTable *FontManager::family_shell(const std::string &font_id, size_t n_files, uint32_t plane) const
{
	if (parent_)
		return parent_->family_shell(font_id, n_files, plane);
	std::lock_guard<std::mutex> lock(family_mu_);
	std::unique_ptr<FamilyTable> &slot = family_shells_[FamilyKey(font_id, plane)];
	if (!slot || slot->n_files != n_files) {
		slot = std::make_unique<FamilyTable>();
		slot->serial = next_family_serial();
		slot->n_files = n_files;
		slot->plane = plane;
	}
	return slot.get();
}

const FontManager::FamilyTable *FontManager::family_table(const std::string &font_id, std::string *err, uint32_t plane) const
{
	const FontEntry *it = find_font(font_id, err);
	if (!it)
		return nullptr;
	if (it->second.files().size() > 0x10000) {
		if (err)
			*err = "font " + font_id + ": more than 65536 files";
		return nullptr;
	}
	if (parent_) // (a lane of a multi-device run: the table is the font id's, whatever share of its blocks the lane renders)
		return parent_->family_table(font_id, err, plane);
	const auto &files = it->second.files();
	std::lock_guard<std::mutex> lock(family_mu_);
	std::unique_ptr<FamilyTable> &slot = family_tables_[FamilyKey(font_id, plane)];
	if (slot && slot->n_files == files.size())
		return slot.get();
	std::map<const FontFileEntry *, uint16_t> file_of;
	for (size_t k = 0; k < files.size(); k++)
		file_of.emplace(files[k].get(), (uint16_t)k);
	ResidentBatch all;
	for (const GlyphBlock &b : it->second.blocks()) // (the font id's own blocks, not a rank's share of them)
		for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE && b.start_index >> 16 == plane; ci++)
			if (const FontFileEntry *f = b.glyphs[ci])
				Renderer::record_resident(f->face(), file_of.at(f), b.start_index + ci, all);
	auto t = std::make_unique<FamilyTable>();
	t->serial = next_family_serial();
	t->n_files = files.size();
	t->plane = plane;
	for (const GlyphJob &j : all.jobs) {
		t->code_point.push_back((uint16_t)j.id);
		t->advance.push_back(j.advance);
	}
	t->font_of = std::move(all.font_of);
	t->glyph_id = std::move(all.glyph_id);
	t->scale = std::move(all.scale);
	t->shift_x = std::move(all.shift_x);
	slot = std::move(t); // (a table built for fewer files is dropped here: its pointers end with it)
	return slot.get();
}

// ---- glyph-level sharding ---------------------------------------------------------------
namespace {

// Estimated raster cost of one recorded glyph: (bitmap area) x (segment count), the w*h*N of SURVEY.md §8e.
// Segments: a quadratic Bezier is halved until |s + e - 2c|^2 <= 0.01 font units^2 (ring.rs:129-131); both
// halves of a quadratic have exactly 1/4 of the parent's deviation, so the depth is uniform and the point
// count is a power of two that follows from the control polygon alone.  Cubics (no fixture font has any) are
// estimated the same way from their larger control deviation.  Area: bounding box of the control points,
// scaled, plus the 3 px buffer on every side (renderer.rs:64-91).
double estimate_cost(const vgsdf_outline_cmd *c, uint32_t n, double scale)
{
	if (n == 0)
		return 1.0;
	double segs = 0, minx = 1e300, miny = 1e300, maxx = -1e300, maxy = -1e300;
	double lx = 0, ly = 0;
	auto grow = [&](double x, double y) {
		minx = std::min(minx, x), maxx = std::max(maxx, x);
		miny = std::min(miny, y), maxy = std::max(maxy, y);
	};
	auto pieces = [](double dev2) {
		double k = 1;
		while (dev2 > 0.01 && k < 65536) {
			dev2 /= 16;
			k *= 2;
		}
		return k;
	};
	for (uint32_t i = 0; i < n; i++) {
		const vgsdf_outline_cmd &q = c[i];
		switch (q.kind) {
		case 0: // move_to
			break;
		case 1: // line_to
			segs += 1;
			break;
		case 2: { // quad_to
			const double dx = lx + q.x - 2.0 * q.x1, dy = ly + q.y - 2.0 * q.y1;
			segs += pieces(dx * dx + dy * dy);
			grow(q.x1, q.y1);
			break;
		}
		case 3: { // curve_to
			const double dx = (double)q.x2 + q.x1 - (lx + q.x), dy = (double)q.y2 + q.y1 - (ly + q.y);
			segs += pieces(dx * dx + dy * dy);
			grow(q.x1, q.y1);
			grow(q.x2, q.y2);
			break;
		}
		default: // close: the closing segment
			segs += 1;
			continue;
		}
		grow(q.x, q.y);
		lx = q.x, ly = q.y;
	}
	if (!(maxx >= minx))
		return 1.0;
	const double w = std::ceil((maxx - minx) * scale) + 2 * BUFFER + 1, h = std::ceil((maxy - miny) * scale) + 2 * BUFFER + 1;
	return std::max(1.0, segs) * w * h;
}

} // namespace

namespace {

// longest processing time first; ties by code point, so every rank computes the same assignment
void assign_lpt(GlyphShard &out)
{
	std::vector<std::pair<double, uint32_t>> order; // (cost, code point)
	for (uint32_t cp = 0; cp < 0x10000; cp++)
		if (out.cost[cp] > 0.0)
			order.emplace_back(out.cost[cp], cp);
	std::sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
	out.owner.assign(0x10000, 0xFF);
	out.load.assign(out.world, 0.0);
	for (const auto &e : order) {
		uint32_t best = 0;
		for (uint32_t r = 1; r < out.world; r++)
			if (out.load[r] < out.load[best])
				best = r;
		out.owner[e.second] = (uint8_t)best;
		out.load[best] += e.first;
	}
}

// estimated costs of the mapped glyphs of one block (cheap: table walks, no flattening), first provider wins
void block_costs(const GlyphBlock &b, OutlineBatch &rec, std::vector<double> &cost)
{
	if (b.start_index >= cost.size()) // (a supplementary block: never split, no place in the tables of 65536 code points)
		return;
	for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE; ci++)
		if (const FontFileEntry *f = b.glyphs[ci]) {
			const uint32_t cp = b.start_index + ci;
			rec.clear();
			double c = 1.0;
			if (Renderer::record(f->face(), cp, rec))
				c = estimate_cost(rec.cmds.data(), (uint32_t)rec.cmds.size(), rec.scale[0]);
			cost[cp] = c; // >= 1 for every mapped code point
		}
}

} // namespace

bool FontManager::shard_glyphs(const std::string &font_id, uint32_t world, GlyphShard &out, std::string *err) const
{
	const FontEntry *it = find_font(font_id, err);
	if (!it)
		return false;
	if (world == 0 || world > 254) {
		if (err)
			*err = "shard_glyphs: world must be 1..254";
		return false;
	}
	out.world = world;
	out.cost.assign(0x10000, 0.0);
	OutlineBatch rec;
	for (const GlyphBlock &b : it->second.blocks())
		block_costs(b, rec, out.cost);
	assign_lpt(out);
	return true;
}

// The same table, kept per (font, world, number of files) and built with the blocks spread over the calling thread's
// pool when there is one (a lane asks its parent; the parent fills the cache before it starts the lanes).
const GlyphShard &FontManager::cached_shard(const std::string &font_id, const FontWrapper &font, uint32_t world) const
{
	if (parent_)
		return parent_->cached_shard(font_id, font, world);
	std::lock_guard<std::mutex> lock(shard_mu_);
	ShardEntry &e = shard_cache_[font_id];
	if (e.world == world && e.n_files == font.files().size() && !e.shard.owner.empty())
		return e.shard;
	if (world == 0 || world > 254)
		throw std::runtime_error("glyph shard: world must be 1..254");
	e.world = world;
	e.n_files = font.files().size();
	e.shard.world = world;
	e.shard.cost.assign(0x10000, 0.0);
	const std::vector<GlyphBlock> &blocks = font.blocks();
	if (pool_ && pool_->size() > 1) {
		std::vector<OutlineBatch> recs(pool_->size());
		pool_->run(blocks.size(), [&](size_t i, unsigned wid) { block_costs(blocks[i], recs[wid], e.shard.cost); });
	} else {
		OutlineBatch rec;
		for (const GlyphBlock &b : blocks)
			block_costs(b, rec, e.shard.cost);
	}
	assign_lpt(e.shard);
	return e.shard;
}

void FontManager::set_glyph_shard(uint32_t rank, uint32_t world)
{
	if (world > 254 || (world > 1 && rank >= world))
		throw std::runtime_error("set_glyph_shard: need rank < world <= 254");
	shard_rank_ = rank;
	shard_world_ = world ? world : 1;
	shard_blocks_.clear();
}

const std::vector<GlyphBlock> &FontManager::task_blocks(const std::string &font_id, const FontWrapper &font) const
{
	if (shard_world_ <= 1)
		return font.blocks();
	auto it = shard_blocks_.find(font_id);
	if (it != shard_blocks_.end())
		return it->second; // (every add_* clears this table: invalidate_shards)
	const GlyphShard &sh = cached_shard(font_id, font, shard_world_);
	std::vector<GlyphBlock> blocks = font.blocks(); // copy, then drop what other ranks own
	for (size_t i = 0; i < blocks.size() && blocks[i].start_index < 0x10000; i++) {
		GlyphBlock &b = blocks[i];
		for (uint32_t ci = 0; ci < GLYPH_BLOCK_SIZE; ci++)
			if (b.glyphs[ci] && sh.owner[b.start_index + ci] != shard_rank_) {
				b.glyphs[ci] = nullptr;
				b.count--;
			}
	}
	// a supplementary block is never split: it is one rank's whole, and the other ranks do not list it (no empty file)
	blocks.erase(std::remove_if(blocks.begin(), blocks.end(),
	                            [&](const GlyphBlock &b) { return b.start_index >= 0x10000 && b.start_index / GLYPH_BLOCK_SIZE % shard_world_ != shard_rank_; }),
	             blocks.end());
	return shard_blocks_[font_id] = std::move(blocks);
}

// A run's union switch: handed to the renderer (and its peers) for the run and taken back when it is over, also when it throws,
// with what the pass saw.  The lanes of a multi-device run are inside their parent's.
struct FontManager::UnionRun {
	FontManager &m;
	const Renderer &r;
	UnionRun(FontManager &mgr, const Renderer &ren) : m(mgr), r(ren)
	{
		if (!m.parent_)
			r.set_union_outlines(m.union_outlines_);
	}
	~UnionRun()
	{
		if (m.parent_)
			return;
		r.set_union_outlines(false);
		uint64_t seen[4];
		r.take_union_stats(seen);
		for (int s = 0; s < 4; s++)
			m.union_stats_[s] += seen[s];
	}
};

void FontManager::render_glyphs(Writer &writer, const Renderer &renderer)
{
	const UnionRun union_run(*this, renderer);
	if (renderer.n_devices() > 1 && renderer.mode() == Renderer::Mode::Hip && !parent_) {
		render_glyphs_multi(writer, renderer);
		return;
	}
	// manager.rs:86-97: one task per (font, block); all 256 blocks per font
	std::vector<Todo> tasks;
	for (const auto &[name, font] : fonts()) {
		writer.write_directory(name + "/");
		for (const GlyphBlock &b : task_blocks(name, font))
			tasks.push_back(Todo{&name, b});
	}
	std::memset(reduced_, 0, sizeof reduced_);
	run_tasks(tasks, writer, renderer);
}

void FontManager::render_blocks(Writer &writer, const Renderer &renderer, const std::string &font_id,
                                const std::vector<uint32_t> &block_starts)
{
	std::string err;
	const FontEntry *it = find_font(font_id, &err);
	if (!it)
		throw std::runtime_error(err);
	const UnionRun union_run(*this, renderer);
	const std::vector<GlyphBlock> &blocks = task_blocks(it->first, it->second);
	std::vector<Todo> tasks;
	for (uint32_t start : block_starts) {
		if (!FontWrapper::find_block(it->second.blocks(), start)) // (a supplementary start that is not populated, or the switch off)
			throw std::runtime_error("bad block start " + std::to_string(start));
		if (const GlyphBlock *b = FontWrapper::find_block(blocks, start)) // (nullptr: a supplementary block of another rank)
			tasks.push_back(Todo{&it->first, *b});
	}
	run_tasks(tasks, writer, renderer);
}

void FontManager::run_tasks(std::vector<Todo> &tasks, Writer &writer, const Renderer &renderer)
{
	if (device_front_end_ && renderer.mode() == Renderer::Mode::Hip) {
		run_tasks_device_front_end(tasks, writer, renderer);
		return;
	}
	timings_ = RenderTimings{};
	const double t_start = now_s();
	ThreadPool &tp = pool();
	std::vector<Slice> slices;

	// GPU batch dispatcher (replaces manager.rs:104-121): groups of `batch_blocks_` tasks are
	// tessellated on the pool, packed into page-locked SoA arrays, rendered with ONE device
	// submission, then PBF-encoded on the pool and written in task order.
	for (size_t g0 = 0; g0 < tasks.size(); g0 += batch_blocks_) {
		const size_t g1 = std::min(tasks.size(), g0 + (size_t)batch_blocks_);
		const size_t nb = g1 - g0;

		tessellate_and_pack(tasks, g0, g1, slices, packed_);
		// slices of a task are contiguous and in code point order
		std::vector<std::pair<size_t, size_t>> span(nb, {0, 0});
		for (size_t i = 0; i < slices.size(); i++) {
			auto &sp = span[slices[i].task - g0];
			if (sp.second == 0)
				sp.first = i;
			sp.second = i + 1;
		}
		// In-place assembly (as the device front-end's, fe_assemble_write): the bitmaps are rendered where the blocks'
		// finished PBFs have them.  The host knows every rect here, so it lays the arena out itself: out_off[g] = position
		// of bitmap g, out_off[n] = size of the arena (vgsdf.h allows gaps between the bitmaps).
		std::vector<uint64_t> entry_at; // per slice: first entry; entries of a slice follow each other
		if (in_place_pbf_) {
			const double tl = now_s();
			entry_at.assign(slices.size() + 1, 0);
			uint64_t pos = 0;
			for (size_t i = 0; i < nb; i++)
				for (size_t k = span[i].first; k < span[i].second; k++) {
					const Slice &s = slices[k];
					const GlyphBatch &l = workers_[s.worker].local;
					if (k == span[i].first)
						pos += kPbfHeadRoom + pbf_block_fields(tasks[g0 + i].name->size(), tasks[g0 + i].block.range().size());
					entry_at[k] = pos;
					uint32_t r = s.g_raster;
					for (uint32_t j = s.job0; j < s.job1; j++) {
						const GlyphJob &job = l.jobs[j];
						const PbfEntrySize es = pbf_entry_size(job.id, job.advance, job.has_raster, job.width, job.height, job.x0, job.y0);
						if (job.has_raster)
							packed_.out_off[r++] = pos + es.bitmap_at;
						pos += es.total;
					}
				}
			entry_at[slices.size()] = pos;
			packed_.out_off[packed_.n_raster] = pos;
			packed_.out_bytes = pos;
			packed_.out.ensure((size_t)pos + 1);
			timings_.pack_s += now_s() - tl;
		}
		const double t1 = now_s();

		renderer.render_packed(packed_);
		const double t2 = now_s();
		timings_.device_s += t2 - t1;

		std::vector<std::vector<uint8_t>> encoded(nb);
		struct Piece {
			const uint8_t *p = nullptr;
			size_t n = 0;
		};
		std::vector<Piece> piece(nb);
		uint64_t n_pixels = 0;
		for (const Slice &s : slices) {
			const GlyphBatch &l = workers_[s.worker].local;
			n_pixels += l.out_off[s.raster1] - l.out_off[s.raster0];
		}
		tp.run(nb, [&](size_t i, unsigned) {
			if (in_place_pbf_ && span[i].second > span[i].first) {
				uint8_t *arena = packed_.out.data();
				uint8_t *first = arena + entry_at[span[i].first], *p = first;
				for (size_t k = span[i].first; k < span[i].second; k++) {
					const Slice &s = slices[k];
					const GlyphBatch &l = workers_[s.worker].local;
					for (uint32_t j = s.job0; j < s.job1; j++) {
						const GlyphJob &job = l.jobs[j];
						p += write_pbf_entry_headers(p, job.id, job.advance, job.has_raster, job.width, job.height, job.x0, job.y0);
					}
				}
				uint8_t *file = write_pbf_block_header(first, *tasks[g0 + i].name, tasks[g0 + i].block.range(), (size_t)(p - first));
				piece[i] = Piece{file, (size_t)(p - file)};
				return;
			}
			std::vector<PbfGlyphRef> refs;
			for (size_t k = span[i].first; k < span[i].second; k++) {
				const Slice &s = slices[k];
				const GlyphBatch &l = workers_[s.worker].local;
				uint32_t r = s.raster0;
				for (uint32_t j = s.job0; j < s.job1; j++) {
					const GlyphJob &job = l.jobs[j];
					const uint8_t *bm = nullptr;
					if (job.has_raster) {
						bm = packed_.out.data() + packed_.out_off[s.g_raster + (r - s.raster0)];
						r++;
					}
					refs.push_back(job.to_pbf(bm));
				}
			}
			encoded[i] = PbfGlyphs::encode(*tasks[g0 + i].name, tasks[g0 + i].block.range(), std::move(refs));
			piece[i] = Piece{encoded[i].data(), encoded[i].size()};
		});
		const double t3 = now_s();
		timings_.encode_s += t3 - t2;

		std::string path;
		for (size_t i = 0; i < nb; i++) {
			tasks[g0 + i].block.path_into(*tasks[g0 + i].name, path);
			writer.write_bytes(path, piece[i].p, piece[i].n);
			timings_.pbf_bytes += piece[i].n;
		}
		timings_.write_s += now_s() - t3;

		timings_.blocks += nb;
		uint64_t group_glyphs = 0;
		for (const Slice &s : slices)
			group_glyphs += s.job1 - s.job0;
		timings_.glyphs += group_glyphs;
		if (group_glyphs) {
			timings_.fe_groups++;
			timings_.fe_max_group_glyphs = std::max(timings_.fe_max_group_glyphs, group_glyphs);
		}
		timings_.rasters += packed_.n_raster;
		timings_.pixels += n_pixels;
		timings_.segments += packed_.n_seg;
	}
	timings_.total_s = now_s() - t_start;
}

} // namespace vg
