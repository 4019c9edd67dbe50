// ttf_face.cpp — see ttf_face.hpp.  Behavioural restatement of ttf-parser 0.25.1 for
// static `glyf` fonts: table lookup, cmap formats 0/4/6/10/12/13, hmtx advances, and the
// glyf outline emitter (implied on-curve midpoints in f32, composite transforms in f32).
// All f32 arithmetic is done operation by operation (library built with
// -ffp-contract=off), as Rust does.
#include "ttf_face.hpp"

#include "cff.hpp"
#include "gvar.hpp"

#include <algorithm>
#include <atomic>
#include <map>
#include <cstdlib>
#include <cstring>

namespace vg {

namespace {

// start of the table directory of face 0 (ttf-parser RawFace::parse with index 0): the file itself, or — a font
// collection, magic 'ttcf' — the first face the collection lists; npos for any other magic than 0x00010000 / 'true' / 'OTTO'
size_t face_directory(Bytes file)
{
	constexpr size_t npos = (size_t)-1;
	auto is_face = [](uint32_t m) { return m == 0x00010000u || m == 0x74727565u || m == 0x4F54544Fu; };
	if (!file.has(0, 4))
		return npos;
	const uint32_t magic = file.u32(0);
	if (is_face(magic))
		return 0;
	if (magic != 0x74746366u || !file.has(4, 8)) // 'ttcf', version, numFonts
		return npos;
	// RawFace::parse reads the WHOLE offsets[numFonts] array (out of bounds: no face) and takes the face's offset relative
	// to the end of that array (`checked_sub`): a face inside the header or the array is refused
	const uint64_t n_fonts = file.u32(8);
	if (n_fonts == 0 || 4 * n_fonts > file.size() || !file.has(12, (size_t)(4 * n_fonts)))
		return npos;
	const size_t at = file.u32(12);
	if (at < 12 + 4 * n_fonts || !file.has(at, 4) || !is_face(file.u32(at))) // (a face is not a collection)
		return npos;
	return at;
}

Bytes find_table(Bytes file, const char tag[4])
{
	const size_t dir = face_directory(file);
	if (dir == (size_t)-1 || !file.has(dir, 12))
		return {};
	const uint16_t n = file.u16(dir + 4);
	for (uint16_t i = 0; i < n; i++) {
		const size_t rec = dir + 12 + (size_t)i * 16;
		if (!file.has(rec, 16))
			return {};
		if (std::memcmp(file.data() + rec, tag, 4) == 0)
			return file.sub(file.u32(rec + 8), file.u32(rec + 12));
	}
	return {};
}

} // namespace

std::optional<Face> Face::parse(const uint8_t *data, size_t len) { return parse_impl(data, len, nullptr, nullptr); }

std::optional<Face> Face::parse_at(const uint8_t *data, size_t len, const std::vector<int16_t> &coords, std::string *err, bool gvar_advances)
{
	auto f = parse_impl(data, len, &coords, err);
	if (f)
		f->gvar_advances_ = gvar_advances; // (before the face is shared: G7 holds for everything built from it)
	return f;
}

namespace {
// the axes of a readable `fvar` (version 1.0, at least one axis, the axis records of 20 bytes each inside the table), 0: none
uint32_t fvar_axes(Bytes fvar, size_t &axes_at)
{
	if (!fvar.has(0, 10) || fvar.u32(0) != 0x00010000u)
		return 0;
	axes_at = fvar.u16(4);
	const uint32_t n_axes = fvar.u16(8);
	return n_axes != 0 && fvar.has(axes_at, (size_t)n_axes * 20) ? n_axes : 0;
}
float fixed_to_float(uint32_t v) { return (float)(int32_t)v / 65536.0f; }
} // namespace

bool read_variation_axes(const uint8_t *data, size_t len, std::vector<VariationAxis> &axes, std::vector<NamedInstance> *instances)
{
	const Bytes fvar = find_table(Bytes(data, len), "fvar");
	size_t axes_at = 0;
	const uint32_t n = fvar_axes(fvar, axes_at);
	if (!n)
		return false;
	axes.clear();
	for (uint32_t i = 0; i < n; i++) {
		const size_t at = axes_at + (size_t)i * 20;
		VariationAxis a;
		std::memcpy(a.tag, fvar.data() + at, 4);
		a.min = fixed_to_float(fvar.u32(at + 4)), a.def = fixed_to_float(fvar.u32(at + 8)), a.max = fixed_to_float(fvar.u32(at + 12));
		axes.push_back(a);
	}
	if (instances) {
		instances->clear();
		if (fvar.has(0, 16)) {
			const size_t axis_size = fvar.u16(10), n_inst = fvar.u16(12), inst_size = fvar.u16(14);
			const size_t first = axes_at + (size_t)n * axis_size;
			for (size_t k = 0; k < n_inst && inst_size >= 4 + (size_t)n * 4; k++) {
				const size_t at = first + k * inst_size;
				if (!fvar.has(at, inst_size))
					break;
				NamedInstance ni;
				ni.name_id = fvar.u16(at);
				for (uint32_t i = 0; i < n; i++)
					ni.coords.push_back(fixed_to_float(fvar.u32(at + 4 + (size_t)i * 4)));
				if (inst_size >= 6 + (size_t)n * 4)
					ni.ps_name_id = fvar.u16(at + 4 + (size_t)n * 4);
				instances->push_back(std::move(ni));
			}
		}
	}
	return true;
}

bool named_instance_ps_names(const uint8_t *data, size_t len, const std::vector<NamedInstance> &instances, std::string &family,
                             std::vector<std::string> &ps_names)
{
	const auto face = Face::parse(data, len);
	if (!face)
		return false;
	std::map<uint16_t, std::string> names;
	for (auto &kv : face->names())
		names[kv.first] = std::move(kv.second);
	family = names.count(1) ? names[1] : std::string();
	std::string prefix = names.count(25) ? names[25] : std::string();
	if (prefix.empty())
		for (const char c : family)
			if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9'))
				prefix.push_back(c);
	ps_names.clear();
	for (const NamedInstance &ni : instances) {
		if (ni.ps_name_id != 0xFFFF && names.count(ni.ps_name_id)) {
			ps_names.push_back(names[ni.ps_name_id]);
			continue;
		}
		std::string ps = prefix + "-";
		if (names.count(ni.name_id))
			for (const char c : names[ni.name_id])
				if (c != ' ')
					ps.push_back(c);
		ps_names.push_back(std::move(ps));
	}
	return true;
}

int16_t normalize_axis_value(const VariationAxis &axis, float v)
{
	v = v < axis.min ? axis.min : v > axis.max ? axis.max : v;
	float n;
	if (v == axis.def)
		n = 0.0f;
	else if (v < axis.def)
		n = (v - axis.def) / (axis.def - axis.min);
	else
		n = (v - axis.def) / (axis.max - axis.def);
	n = n < -1.0f ? -1.0f : n > 1.0f ? 1.0f : n;
	return (int16_t)(n * 16384.0f); // (|n| <= 1, or NaN from a degenerate axis: sent to 0)
}

void apply_avar(const uint8_t *data, size_t len, std::vector<int16_t> &coords)
{
	const Bytes avar = find_table(Bytes(data, len), "avar");
	if (!avar.has(0, 8) || avar.u32(0) != 0x00010000u || avar.u16(6) != coords.size())
		return;
	size_t at = 8;
	for (int16_t &coord : coords) {
		if (!avar.has(at, 2))
			return;
		const size_t n = avar.u16(at);
		if (!avar.has(at + 2, n * 4))
			return;
		// (i64: the product of two differences of i16 values does not fit i32; a result outside i16 is discarded below)
		auto from = [&](size_t i) { return (int64_t)avar.i16(at + 2 + i * 4); };
		auto to = [&](size_t i) { return (int64_t)avar.i16(at + 4 + i * 4); };
		const int64_t v = coord;
		int64_t r = v;
		if (n == 1) {
			r = v - from(0) + to(0);
		} else if (n > 1) {
			if (v <= from(0)) {
				r = v - from(0) + to(0);
			} else {
				size_t i = 1;
				while (i < n && v > from(i))
					i++;
				if (i == n)
					i = n - 1;
				if (v >= from(i)) {
					r = v - from(i) + to(i);
				} else if (from(i - 1) == from(i)) {
					r = to(i - 1);
				} else {
					const int64_t d = from(i) - from(i - 1);
					r = to(i - 1) + ((to(i) - to(i - 1)) * (v - from(i - 1)) + d / 2) / d;
				}
			}
		}
		if (r >= -32768 && r <= 32767)
			coord = (int16_t)r;
		at += 2 + n * 4;
	}
}

std::optional<Face> Face::parse_impl(const uint8_t *data, size_t len, const std::vector<int16_t> *at_coords, std::string *err)
{
	auto refuse = [&](const char *why) {
		if (err)
			*err = why;
		return std::nullopt;
	};
	Bytes file(data, len);
	const Bytes head = find_table(file, "head"), maxp = find_table(file, "maxp"),
	            hhea = find_table(file, "hhea");
	if (!head.has(0, 54) || !maxp.has(0, 6) || !hhea.has(0, 36))
		return refuse("font parse failed");
	Face f;
	f.units_per_em_ = head.u16(18);
	if (f.units_per_em_ < 16 || f.units_per_em_ > 16384)
		return refuse("font parse failed");
	f.loca_long_ = head.i16(50) != 0;
	f.num_glyphs_ = maxp.u16(4);
	f.num_hmetrics_ = hhea.u16(34);
	f.hmtx_ = find_table(file, "hmtx");
	f.loca_ = find_table(file, "loca");
	f.glyf_ = find_table(file, "glyf");
	if (!f.loca_.empty()) {
		size_t want = (size_t)f.num_glyphs_ + 1;
		if (f.num_glyphs_ == 0xFFFF)
			want = 0xFFFF;
		f.loca_entries_ = std::min(want, f.loca_.size() / (f.loca_long_ ? 4u : 2u));
	}
	f.name_ = find_table(file, "name");
	if (const Bytes cff = find_table(file, "CFF "); !cff.empty()) {
		if (auto t = CffTable::parse(cff))
			f.cff_ = std::make_shared<const CffTable>(std::move(*t));
		else
			f.cff_unreadable_ = true;
	}
	if (const Bytes cff2 = find_table(file, "CFF2"); !f.cff_ && !cff2.empty()) {
		// ttf-parser: glyf, then cff1, then cff2 — drawn at the face's variation coordinates, which the reference
		// leaves at their defaults: one (zero) coordinate per `fvar` axis, at most 64, none without a readable `fvar`
		// (parse_at: the coordinates it was given, checked below to be as many)
		size_t axes_at = 0;
		std::vector<int16_t> coords(std::min<uint32_t>(fvar_axes(find_table(file, "fvar"), axes_at), 64), 0);
		if (at_coords && at_coords->size() == coords.size())
			coords = *at_coords;
		if (auto t = CffTable::parse2(cff2, coords))
			f.cff_ = std::make_shared<const CffTable>(std::move(*t));
		else
			f.cff_unreadable_ = true;
	}
	const Bytes cmap = find_table(file, "cmap");
	f.has_cmap_ = cmap.has(0, 4);
	f.cmap_table_ = cmap;
	if (cmap.has(0, 4)) {
		const uint16_t n = cmap.u16(2);
		for (uint16_t i = 0; i < n; i++) {
			const size_t rec = 4 + (size_t)i * 8;
			if (!cmap.has(rec, 8))
				break;
			CmapSubtable st;
			st.platform = cmap.u16(rec);
			st.encoding = cmap.u16(rec + 2);
			st.data = cmap.from(cmap.u32(rec + 4));
			st.offset = cmap.u32(rec + 4);
			if (st.data.has(0, 2))
				st.format = st.data.u16(0);
			f.cmap_.push_back(st);
		}
	}
	if (at_coords) {
		size_t axes_at = 0;
		const uint32_t n_axes = std::min<uint32_t>(fvar_axes(find_table(file, "fvar"), axes_at), 64);
		if (!n_axes)
			return refuse("a position needs a readable fvar table, and this file has none");
		if (f.has_glyf_outlines()) {
			// (gvar's axisCount is fvar's own, not the 64 the coordinates are counted to: a file of more axes is refused below)
			if (auto g = GvarTable::parse(find_table(file, "gvar"), n_axes))
				f.gvar_ = std::make_shared<const GvarTable>(std::move(*g));
			else
				return refuse("a position for a face with glyf outlines needs a readable gvar table (version 1.0, as many axes as fvar), and this file has none");
		}
		if (at_coords->size() != n_axes)
			return refuse("the number of coordinates is not the number of fvar axes (at most 64 are counted)");
		f.at_position_ = true;
		f.coords_ = *at_coords;
		// HVAR: majorVersion, minorVersion, the store's offset, the advance map's (0: none), two more maps
		const Bytes hvar = find_table(file, "HVAR");
		if (hvar.has(0, 20) && hvar.u16(0) == 1 && hvar.size() <= 0xFFFFFFFFu) {
			const size_t store = hvar.u32(4);
			const Bytes st = hvar.from(store);
			if (st.has(0, 8)) {
				if (st.u16(0) != 1)
					return refuse("HVAR: an ItemVariationStore of a format other than 1");
				const size_t regions_at = st.u32(2);
				const uint32_t n_data = st.u16(6);
				if (st.has(8, (size_t)n_data * 4) && st.has(regions_at, 4) &&
				    st.has(regions_at + 4, (size_t)st.u16(regions_at) * st.u16(regions_at + 2) * 6)) {
					for (uint32_t d = 0; d < n_data; d++) {
						const size_t at = st.u32(8 + (size_t)d * 4);
						if (st.has(at, 6) && (st.u16(at + 2) & 0x8000u))
							return refuse("HVAR: an ItemVariationData with 32-bit deltas (LONG_WORDS)");
					}
					const Bytes list = st.from(regions_at);
					const uint32_t n_regions = list.u16(2);
					for (uint32_t r = 0; r < n_regions; r++)
						f.hvar_scalars_.push_back(variation_region_factor(list, r, f.coords_));
					f.hvar_ = hvar;
					f.hvar_store_ = (uint32_t)store;
					f.hvar_map_ = hvar.u32(8);
				}
			}
		}
	}
	return f;
}

// ---- name ------------------------------------------------------------------------------
std::vector<std::pair<uint16_t, std::string>> Face::names() const
{
	std::vector<std::pair<uint16_t, std::string>> out;
	if (!name_.has(0, 6))
		return out;
	const uint16_t version = name_.u16(0), count = name_.u16(2);
	const size_t storage_off = name_.u16(4);
	if (version > 1 || !name_.has(6, (size_t)count * 12))
		return out;
	const Bytes storage = name_.from(std::max(storage_off, (size_t)6 + (size_t)count * 12));
	for (uint16_t i = 0; i < count; i++) {
		const size_t rec = 6 + (size_t)i * 12;
		const uint16_t platform = name_.u16(rec), encoding = name_.u16(rec + 2), name_id = name_.u16(rec + 6);
		const size_t len = name_.u16(rec + 8), off = name_.u16(rec + 10);
		if (!storage.has(off, len))
			break; // the crate's iterator ends at the first record whose bytes are out of range
		std::string text;
		const bool unicode = platform == 0 || (platform == 3 && (encoding == 0 || encoding == 1));
		if (unicode) { // String::from_utf16 over the big-endian units; an unpaired surrogate -> None -> ""
			bool ok = true;
			for (size_t k = 0; k + 1 < len && ok; k += 2) {
				uint32_t c = storage.u16(off + k);
				if (c >= 0xD800 && c <= 0xDBFF) {
					const uint32_t lo = (k + 3 < len) ? storage.u16(off + k + 2) : 0;
					if (lo >= 0xDC00 && lo <= 0xDFFF) {
						c = 0x10000 + ((c - 0xD800) << 10) + (lo - 0xDC00);
						k += 2;
					} else {
						ok = false;
					}
				} else if (c >= 0xDC00 && c <= 0xDFFF) {
					ok = false;
				}
				if (!ok)
					break;
				if (c < 0x80) {
					text.push_back((char)c);
				} else if (c < 0x800) {
					text.push_back((char)(0xC0 | (c >> 6)));
					text.push_back((char)(0x80 | (c & 63)));
				} else if (c < 0x10000) {
					text.push_back((char)(0xE0 | (c >> 12)));
					text.push_back((char)(0x80 | ((c >> 6) & 63)));
					text.push_back((char)(0x80 | (c & 63)));
				} else {
					text.push_back((char)(0xF0 | (c >> 18)));
					text.push_back((char)(0x80 | ((c >> 12) & 63)));
					text.push_back((char)(0x80 | ((c >> 6) & 63)));
					text.push_back((char)(0x80 | (c & 63)));
				}
			}
			if (!ok)
				text.clear();
		}
		out.emplace_back(name_id, std::move(text));
	}
	return out;
}

// ---- hmtx ------------------------------------------------------------------------------
std::optional<uint16_t> Face::glyph_hor_advance(uint16_t gid) const
{
	if (hmtx_.empty() || num_hmetrics_ == 0 || num_glyphs_ == 0 || gid >= num_glyphs_)
		return std::nullopt;
	if (!hmtx_.has(0, (size_t)num_hmetrics_ * 4))
		return std::nullopt;
	// fewer long metrics than glyphs: the last advance applies to the rest
	const size_t i = std::min<size_t>(gid, (size_t)num_hmetrics_ - 1);
	if (!at_position_)
		return hmtx_.u16(i * 4);
	// the crate's variable path: f32 throughout, `+ 0.5` for rounding, u16::try_from of the truncated value
	float a = (float)hmtx_.u16(i * 4);
	if (const auto delta = hvar_advance_delta(gid)) {
		a += *delta + 0.5f;
	} else if (advances_by_gvar()) { // G7
		float d;
		if (gvar_advance_delta(gid, d) != kGvarAdvanceMalformed)
			a += d + 0.5f;
	}
	if (!(a > -1.0f && a < 65536.0f))
		return std::nullopt;
	return (uint16_t)(int32_t)a;
}

std::vector<uint16_t> Face::hor_advances(uint32_t n) const
{
	std::vector<uint16_t> out(n, 0);
	for (uint32_t g = 0; g < n && g <= 0xFFFFu; g++)
		out[g] = glyph_hor_advance((uint16_t)g).value_or(0);
	return out;
}

std::optional<float> Face::hvar_advance_delta(uint16_t gid) const
{
	if (hvar_.empty())
		return std::nullopt;
	uint32_t outer = 0, inner = gid;
	if (hvar_map_ != 0) { // DeltaSetIndexMap: format, entryFormat, mapCount (u16: format 0, u32: format 1), entries
		const Bytes m = hvar_.from(hvar_map_);
		if (!m.has(0, 2))
			return std::nullopt;
		const uint32_t format = m.u8(0), ef = m.u8(1);
		if (format > 1 || !m.has(2, format ? 4 : 2))
			return std::nullopt;
		const uint32_t count = format ? m.u32(2) : m.u16(2);
		if (count == 0)
			return std::nullopt;
		const size_t entry_size = ((ef >> 4) & 3) + 1, at = (format ? 6 : 4) + entry_size * std::min<uint32_t>(gid, count - 1);
		if (!m.has(at, entry_size))
			return std::nullopt;
		uint32_t n = 0;
		for (size_t k = 0; k < entry_size; k++)
			n = (n << 8) | m.u8(at + k);
		const uint32_t bits = (ef & 15) + 1;
		outer = n >> bits, inner = n & ((1u << bits) - 1);
		if (outer > 0xFFFFu)
			return std::nullopt;
	}
	const Bytes st = hvar_.from(hvar_store_);
	if (outer >= st.u16(6))
		return std::nullopt;
	const size_t at = st.u32(8 + (size_t)outer * 4);
	if (!st.has(at, 6))
		return std::nullopt;
	const uint32_t item_count = st.u16(at), words = st.u16(at + 2), n_cols = st.u16(at + 4); // (no LONG_WORDS: parse_at)
	if (!st.has(at + 6, (size_t)n_cols * 2) || inner >= item_count || words > n_cols)
		return std::nullopt;
	const size_t row = at + 6 + (size_t)n_cols * 2 + (size_t)inner * (words + n_cols);
	if (!st.has(row, (size_t)words + n_cols))
		return std::nullopt;
	float delta = 0.0f;
	size_t p = row;
	for (uint32_t c = 0; c < n_cols; c++) {
		const uint32_t region = st.u16(at + 6 + (size_t)c * 2);
		float num;
		if (c < words)
			num = (float)st.i16(p), p += 2;
		else
			num = (float)(int8_t)st.u8(p), p += 1;
		delta += num * (region < hvar_scalars_.size() ? hvar_scalars_[region] : 0.0f);
	}
	return delta;
}

// ---- cmap ------------------------------------------------------------------------------
bool Face::CmapSubtable::is_unicode() const
{
	switch (platform) {
	case 0:
		return true;
	case 3:
		if (encoding == 1)
			return true;
		return encoding == 10 && (format == 12 || format == 13);
	default:
		return false;
	}
}

namespace {

struct Format4 {
	Bytes d;
	size_t segs = 0, ends = 0, starts = 0, deltas = 0, offsets = 0;
	bool ok = false;
	explicit Format4(Bytes data) : d(data)
	{
		if (!d.has(0, 14))
			return;
		const uint16_t x2 = d.u16(6);
		if (x2 < 2)
			return;
		segs = x2 / 2;
		ends = 14;
		starts = ends + segs * 2 + 2;
		deltas = starts + segs * 2;
		offsets = deltas + segs * 2;
		ok = d.has(offsets, segs * 2);
	}
};

} // namespace

std::optional<uint16_t> Face::CmapSubtable::glyph_index(uint32_t cp) const
{
	switch (format) {
	case 0: {
		if (cp >= 256 || !data.has(6, 256))
			return std::nullopt;
		const uint8_t g = data.u8(6 + cp);
		if (g == 0)
			return std::nullopt;
		return g;
	}
	case 4: {
		const Format4 t(data);
		if (!t.ok || cp > 0xFFFF)
			return std::nullopt;
		const uint16_t c = (uint16_t)cp;
		size_t lo = 0, hi = t.segs;
		while (lo < hi) { // the crate's own bisection over endCode[]
			const size_t mid = (lo + hi) / 2;
			if (data.u16(t.ends + mid * 2) < c) {
				lo = mid + 1;
				continue;
			}
			const uint16_t first = data.u16(t.starts + mid * 2);
			if (first > c) {
				hi = mid;
				continue;
			}
			const uint16_t range_off = data.u16(t.offsets + mid * 2);
			const uint16_t delta = data.u16(t.deltas + mid * 2);
			if (range_off == 0)
				return (uint16_t)(c + delta);
			if (range_off == 0xFFFF)
				return std::nullopt;
			const uint32_t twice = ((uint32_t)c - first) * 2;
			if (twice > 0xFFFF)
				return std::nullopt;
			// u16 wrapping position arithmetic, relative to the subtable start
			const uint16_t pos = (uint16_t)((uint16_t)(t.offsets + mid * 2) + (uint16_t)twice + range_off);
			if (!data.has(pos, 2))
				return std::nullopt;
			const uint16_t raw = data.u16(pos);
			if (raw == 0)
				return std::nullopt;
			const int16_t id = (int16_t)(uint16_t)(raw + delta);
			if (id < 0)
				return std::nullopt;
			return (uint16_t)id;
		}
		return std::nullopt;
	}
	case 6: {
		if (cp > 0xFFFF || !data.has(0, 10))
			return std::nullopt;
		const uint32_t first = data.u16(6), count = data.u16(8);
		if (cp < first || cp - first >= count || !data.has(10 + (size_t)(cp - first) * 2, 2))
			return std::nullopt;
		return data.u16(10 + (size_t)(cp - first) * 2);
	}
	case 10: {
		if (!data.has(0, 20))
			return std::nullopt;
		const uint32_t first = data.u32(12), count = data.u32(16);
		if (cp < first || cp - first >= count || !data.has(20 + (size_t)(cp - first) * 2, 2))
			return std::nullopt;
		return data.u16(20 + (size_t)(cp - first) * 2);
	}
	case 12:
	case 13: {
		if (!data.has(0, 16))
			return std::nullopt;
		const uint32_t n = data.u32(12);
		if (!data.has(16, (size_t)n * 12))
			return std::nullopt;
		size_t lo = 0, hi = n;
		while (lo < hi) {
			const size_t mid = lo + (hi - lo) / 2, g = 16 + mid * 12;
			if (data.u32(g) > cp)
				hi = mid;
			else if (data.u32(g + 4) < cp)
				lo = mid + 1;
			else {
				uint64_t id = data.u32(g + 8);
				if (format == 12) {
					id += cp;
					if (id > 0xFFFFFFFFull)
						return std::nullopt;
					id -= data.u32(g);
				}
				if (id > 0xFFFF)
					return std::nullopt;
				return (uint16_t)id;
			}
		}
		return std::nullopt;
	}
	default: // 2, 8, 14: not produced by any fixture; treated as "no mapping"
		return std::nullopt;
	}
}

template <class F> void Face::CmapSubtable::for_each_codepoint(F &&f) const
{
	switch (format) {
	case 0:
		if (data.has(6, 256))
			for (uint32_t c = 0; c < 256; c++)
				if (data.u8(6 + c) != 0)
					f(c);
		break;
	case 4: {
		const Format4 t(data);
		if (!t.ok)
			break;
		for (size_t s = 0; s < t.segs; s++) {
			const uint32_t a = data.u16(t.starts + s * 2), b = data.u16(t.ends + s * 2);
			if (a == 0xFFFF && b == 0xFFFF)
				break;
			for (uint32_t c = a; c <= b; c++)
				f(c);
		}
		break;
	}
	case 6:
		if (data.has(0, 10)) {
			const uint32_t first = data.u16(6), count = data.u16(8);
			for (uint32_t k = 0; k < count && first + k <= 0xFFFF; k++)
				f(first + k);
		}
		break;
	case 10:
		if (data.has(0, 20)) {
			const uint32_t first = data.u32(12), count = data.u32(16);
			for (uint32_t k = 0; k < count && first + k >= first; k++)
				f(first + k);
		}
		break;
	case 12:
	case 13:
		if (data.has(0, 16)) {
			const uint32_t n = data.u32(12);
			if (!data.has(16, (size_t)n * 12))
				break;
			for (uint32_t k = 0; k < n; k++) {
				const size_t g = 16 + (size_t)k * 12;
				for (uint64_t c = data.u32(g), e = data.u32(g + 4); c <= e; c++)
					f((uint32_t)c);
			}
		}
		break;
	default:
		break;
	}
}

std::optional<uint16_t> Face::glyph_index(uint32_t cp) const
{
	for (const CmapSubtable &st : cmap_) {
		if (st.format == 0xFFFF || !st.is_unicode())
			continue;
		if (auto g = st.glyph_index(cp))
			return g;
	}
	return std::nullopt;
}

std::vector<uint32_t> Face::unicode_codepoints() const
{
	std::vector<uint32_t> cps;
	for (const CmapSubtable &st : cmap_) {
		if (st.format == 0xFFFF || !st.is_unicode())
			continue;
		st.for_each_codepoint([&](uint32_t c) {
			if (st.glyph_index(c)) // metadata.rs:111-113
				cps.push_back(c);
		});
	}
	std::sort(cps.begin(), cps.end());
	cps.erase(std::unique(cps.begin(), cps.end()), cps.end());
	return cps;
}

// The description of cmap and hmtx for the device.  On REGULAR tables the bisection of glyph_index and the enumeration of
// for_each_codepoint agree about the segment or group that holds a code point, which is what the device's statement rests on;
// a table that is not regular is refused here and its family is built by the reader above.
const FamilyTables &Face::family_tables() const
{
	FamilyCell &cell = *family_;
	std::call_once(cell.once, [&] {
		FamilyTables &t = cell.tables;
		t.cmap = cmap_table_.data(), t.cmap_len = (uint32_t)std::min<size_t>(cmap_table_.size(), 0xFFFFFFFFu);
		t.hmtx = hmtx_.data(), t.hmtx_len = (uint32_t)std::min<size_t>(hmtx_.size(), 0xFFFFFFFFu);
		t.units_per_em = units_per_em_, t.num_glyphs = num_glyphs_, t.num_hmetrics = num_hmetrics_;
		if (cmap_table_.size() > 0xFFFFFFFFu || hmtx_.size() > 0xFFFFFFFFu)
			return;
		for (const CmapSubtable &st : cmap_) {
			if (st.format == 0xFFFF || !st.is_unicode())
				continue;
			const Bytes &d = st.data;
			switch (st.format) {
			case 0:
			case 6:
			case 10:
				break;
			case 4: {
				const Format4 f4(d);
				if (!f4.ok)
					return;
				for (size_t k = 0; k < f4.segs; k++) {
					const uint16_t a = d.u16(f4.starts + k * 2), b = d.u16(f4.ends + k * 2);
					if (a > b || (k && a <= d.u16(f4.ends + (k - 1) * 2)))
						return;
				}
				break;
			}
			case 12:
			case 13: {
				if (!d.has(0, 16))
					return;
				const uint32_t n = d.u32(12);
				if (!d.has(16, (size_t)n * 12))
					return;
				for (uint32_t k = 0; k < n; k++) {
					const size_t g = 16 + (size_t)k * 12;
					if (d.u32(g) > d.u32(g + 4) || (k && d.u32(g) <= d.u32(g - 12 + 4)))
						return;
				}
				break;
			}
			default: // 2, 8, 14: glyph_index has no value for them
				continue;
			}
			t.subtable_off.push_back(st.offset);
			t.subtable_format.push_back(st.format);
		}
		t.ok = t.subtable_off.size() <= 0xFFFFu;
		if (!hvar_.empty()) {
			// An advance map outside the table is what vgsdf_family_create_tables_var refuses.  A map of a format above 1 and
			// more word deltas than regions are refused here as well although the kernel answers both as the reader does, with
			// "no delta" (tests/test_gpu_family_tables_var_regimes.py holds it to that): no font tool writes such a table, and
			// a font id that has one goes the road every other refusal goes instead of being a case of its own on the device
			bool fits = true;
			if (hvar_map_ != 0) {
				const Bytes m = hvar_.from(hvar_map_);
				fits = hvar_map_ < hvar_.size() && !(m.has(0, 1) && m.u8(0) > 1);
			}
			const Bytes st = hvar_.from(hvar_store_);
			for (uint32_t d = 0, n_data = st.u16(6); d < n_data; d++) {
				const size_t at = st.u32(8 + (size_t)d * 4);
				if (st.has(at, 6) && st.u16(at + 2) > st.u16(at + 4))
					fits = false;
			}
			if (!fits) {
				t.hvar_refused = true;
				t.ok = false;
				return;
			}
			t.hvar = hvar_.data(), t.hvar_len = (uint32_t)hvar_.size();
			t.hvar_store = hvar_store_, t.hvar_map = hvar_map_;
			t.region_scalars = hvar_scalars_;
		}
	});
	return cell.tables;
}

// ---- gvar (gvar.hpp; here and not in a file of its own: this file and cff.cpp are the reader, whoever compiles it) ---
std::optional<GvarTable> GvarTable::parse(Bytes table, uint32_t n_axes)
{
	// majorVersion, minorVersion, axisCount, sharedTupleCount, sharedTuplesOffset, glyphCount, flags, glyphVariationDataArrayOffset
	if (!table.has(0, 20) || table.size() > 0xFFFFFFFFu || table.u32(0) != 0x00010000u || table.u16(4) != n_axes || n_axes == 0)
		return std::nullopt;
	GvarTable t;
	t.table_ = table;
	t.axis_count_ = n_axes;
	t.shared_count_ = table.u16(6);
	t.shared_at_ = table.u32(8);
	t.glyph_count_ = table.u16(12);
	t.long_offsets_ = (table.u16(14) & 1) != 0;
	t.data_at_ = table.u32(16);
	if (!table.has(t.shared_at_, (size_t)t.shared_count_ * n_axes * 2) ||
	    !table.has(20, ((size_t)t.glyph_count_ + 1) * (t.long_offsets_ ? 4u : 2u)))
		return std::nullopt;
	return t;
}

namespace {

// G2: the packed point numbers of b from p on, one after the other; false: they leave b, or do not ascend
struct PointNumberStream {
	Bytes b;
	size_t p = 0;
	uint32_t count = 0, got = 0, run_left = 0;
	uint16_t number = 0;
	bool words = false, all = false;
	bool open(Bytes bytes, size_t at)
	{
		b = bytes, p = at;
		if (!b.has(p, 1))
			return false;
		count = b.u8(p++);
		if (count == 0) {
			all = true;
		} else if (count & 0x80u) {
			if (!b.has(p, 1))
				return false;
			count = ((count & 0x7Fu) << 8) | b.u8(p++);
		}
		return true;
	}
	bool next(uint16_t &out)
	{
		if (run_left == 0) {
			if (!b.has(p, 1))
				return false;
			const uint8_t control = b.u8(p++);
			words = (control & 0x80) != 0;
			run_left = (control & 0x7Fu) + 1;
		}
		if (!b.has(p, words ? 2 : 1))
			return false;
		const uint16_t step = words ? b.u16(p) : b.u8(p);
		p += words ? 2 : 1;
		const uint16_t following = (uint16_t)(number + step);
		if (got && following <= number)
			return false;
		number = out = following;
		got++, run_left--;
		return true;
	}
};
// the numbers at b[p...] are well formed; all: they stand for every point; end: the first byte behind them
bool check_point_numbers(Bytes b, size_t p, bool &all, size_t &end)
{
	PointNumberStream s;
	if (!s.open(b, p))
		return false;
	uint16_t number;
	while (s.got < s.count)
		if (!s.next(number))
			return false;
	all = s.all, end = s.p;
	return true;
}

// G3: the packed deltas of a tuple as one stream of values
struct DeltaStream {
	Bytes b;
	size_t p;
	uint32_t left = 0; // of the run in hand
	uint8_t control = 0;
	bool next(int32_t &v)
	{
		if (left == 0) {
			if (!b.has(p, 1))
				return false;
			control = b.u8(p++);
			left = (control & 0x3Fu) + 1;
		}
		left--;
		if (control & 0x80) {
			v = 0;
		} else if (control & 0x40) {
			if (!b.has(p, 2))
				return false;
			v = b.i16(p), p += 2;
		} else {
			if (!b.has(p, 1))
				return false;
			v = (int8_t)b.u8(p), p += 1;
		}
		return true;
	}
};

// G5: what a point at p takes from the touched points at pa (before it) and pb (behind it) of its contour
float inferred(int32_t p, int32_t pa, int32_t pb, float da, float db)
{
	if (pa == pb)
		return da == db ? da : 0.0f;
	if (p <= std::min(pa, pb))
		return pa < pb ? da : db;
	if (p >= std::max(pa, pb))
		return pa > pb ? da : db;
	const float d = (float)(p - pa) / (float)(pb - pa);
	return (1.0f - d) * da + d * db;
}

} // namespace

// The one walk over a glyph id's tuples, rules G1 to G4 and nothing else: accumulate and phantom_sums are this walk with a visitor
// each, so what is malformed to the outline is malformed to the advances (G7).  Of every tuple whose scalar is not zero
// visit(scalar, all, numbers_in, numbers_at, deltas): all, or the tuple's point numbers are those of numbers_in from numbers_at
// on (check_point_numbers has passed them); deltas (a DeltaStream) stands at the tuple's first delta.  The visitor returns
// false for malformed.  Tuples::None: no variation data (nothing was visited), Applied, or Malformed.
template <class Visit> GvarTable::Tuples GvarTable::applied_tuples(uint16_t gid, const std::vector<int16_t> &coords, Visit &&visit) const
{
	if (gid >= glyph_count_ || coords.size() != axis_count_)
		return Tuples::None;
	// G1
	size_t from, to;
	if (long_offsets_)
		from = table_.u32(20 + (size_t)gid * 4), to = table_.u32(24 + (size_t)gid * 4);
	else
		from = (size_t)table_.u16(20 + (size_t)gid * 2) * 2, to = (size_t)table_.u16(22 + (size_t)gid * 2) * 2;
	if (from == to)
		return Tuples::None;
	if (from > to || !table_.has(data_at_, to))
		return Tuples::Malformed;
	const Bytes d = table_.sub(data_at_ + from, to - from);
	if (!d.has(0, 4))
		return Tuples::Malformed;
	const uint32_t n_tuples = d.u16(0) & 0x0FFFu;
	const bool have_shared = (d.u16(0) & 0x8000u) != 0;
	if (n_tuples == 0)
		return Tuples::None;
	size_t cursor = d.u16(2);
	if (cursor > d.size())
		return Tuples::Malformed;
	bool shared_all = true;
	size_t shared_at = 0;
	if (have_shared) {
		shared_at = cursor;
		if (!check_point_numbers(d, shared_at, shared_all, cursor))
			return Tuples::Malformed;
	}
	size_t h = 4;
	const size_t tuple_bytes = (size_t)axis_count_ * 2;
	for (uint32_t t = 0; t < n_tuples; t++) {
		if (!d.has(h, 4))
			return Tuples::Malformed;
		const size_t size = d.u16(h);
		const uint32_t index = d.u16(h + 2);
		h += 4;
		Bytes peak, start, end;
		if (index & 0x8000u) {
			if (!d.has(h, tuple_bytes))
				return Tuples::Malformed;
			peak = d.sub(h, tuple_bytes);
			h += tuple_bytes;
		} else {
			if ((index & 0x0FFFu) >= shared_count_)
				return Tuples::Malformed;
			peak = table_.sub(shared_at_ + (size_t)(index & 0x0FFFu) * tuple_bytes, tuple_bytes);
		}
		if (index & 0x4000u) {
			if (!d.has(h, 2 * tuple_bytes))
				return Tuples::Malformed;
			start = d.sub(h, tuple_bytes), end = d.sub(h + tuple_bytes, tuple_bytes);
			h += 2 * tuple_bytes;
		}
		if (!d.has(cursor, size))
			return Tuples::Malformed;
		const Bytes data = d.sub(cursor, size);
		cursor += size;
		// G4
		float scalar = 1.0f;
		for (uint32_t i = 0; i < axis_count_ && scalar != 0.0f; i++) {
			const int16_t pk = peak.i16((size_t)i * 2);
			const int16_t st = start.empty() ? std::min<int16_t>(pk, 0) : start.i16((size_t)i * 2);
			const int16_t en = end.empty() ? std::max<int16_t>(pk, 0) : end.i16((size_t)i * 2);
			const float f = axis_factor(coords[i], st, pk, en);
			scalar = f == 0.0f ? 0.0f : scalar * f;
		}
		if (scalar == 0.0f)
			continue;
		// the tuple's point numbers: its own (in its data, the deltas behind them) or the shared ones
		Bytes numbers_in = d;
		size_t numbers_at = shared_at, deltas_at = 0;
		bool all = shared_all;
		if (index & 0x2000u) {
			numbers_in = data, numbers_at = 0;
			if (!check_point_numbers(data, 0, all, deltas_at))
				return Tuples::Malformed;
		}
		DeltaStream deltas{data, deltas_at};
		if (!visit(scalar, all, numbers_in, numbers_at, deltas))
			return Tuples::Malformed;
	}
	return Tuples::Applied;
}

bool GvarTable::accumulate(uint16_t gid, const std::vector<int16_t> &coords, const GvarPoints &pts, std::vector<float> &acc) const
{
	const uint32_t n_all = pts.n + 4;
	acc.assign((size_t)2 * n_all, 0.0f);
	std::vector<float> sx, sy;
	std::vector<uint8_t> mark; // 1: touched, 2: inferred
	std::vector<uint32_t> before, behind;
	const auto tuple = [&](float scalar, bool all, Bytes numbers_in, size_t numbers_at, DeltaStream &deltas) {
		int32_t v;
		if (all) {
			for (int axis = 0; axis < 2; axis++)
				for (uint32_t i = 0; i < n_all; i++) {
					if (!deltas.next(v))
						return false;
					acc[(size_t)2 * i + axis] += (float)v * scalar;
				}
			return true;
		}
		sx.assign(n_all, 0.0f), sy.assign(n_all, 0.0f), mark.assign(n_all, 0);
		for (int axis = 0; axis < 2; axis++) { // the numbers once for x and once for y
			PointNumberStream numbers;
			(void)numbers.open(numbers_in, numbers_at); // (the walk checked them)
			while (numbers.got < numbers.count) {
				uint16_t number = 0;
				if (!numbers.next(number) || !deltas.next(v))
					return false;
				if (number < n_all) // (a number at or past the count names no point)
					(axis ? sy : sx)[number] = (float)v * scalar, mark[number] = 1;
			}
		}
		if (pts.last_of_contour) {
			before.resize(pts.n), behind.resize(pts.n);
			for (uint32_t first = 0; first < pts.n;) {
				uint32_t last = first;
				while (last + 1 < pts.n && !pts.last_of_contour[last])
					last++;
				uint32_t lo = 0xFFFFFFFFu, hi = 0;
				for (uint32_t i = first; i <= last; i++)
					if (mark[i] == 1)
						lo = std::min(lo, i), hi = i;
				if (lo != 0xFFFFFFFFu) {
					// (cyclic: in front of the first touched point lies the last one, behind the last the first)
					for (uint32_t i = first, at = hi; i <= last; i++) {
						if (mark[i] == 1)
							at = i;
						before[i] = at;
					}
					for (uint32_t i = last + 1, at = lo; i-- > first;) {
						if (mark[i] == 1)
							at = i;
						behind[i] = at;
					}
					for (uint32_t i = first; i <= last; i++)
						if (mark[i] == 0) {
							const uint32_t a = before[i], b = behind[i];
							sx[i] = inferred(pts.x[i], pts.x[a], pts.x[b], sx[a], sx[b]);
							sy[i] = inferred(pts.y[i], pts.y[a], pts.y[b], sy[a], sy[b]);
							mark[i] = 2;
						}
				}
				first = last + 1;
			}
		}
		for (uint32_t i = 0; i < n_all; i++)
			if (mark[i])
				acc[(size_t)2 * i] += sx[i], acc[(size_t)2 * i + 1] += sy[i];
		return true;
	};
	return applied_tuples(gid, coords, tuple) != Tuples::Malformed;
}

uint8_t GvarTable::phantom_sums(uint16_t gid, const std::vector<int16_t> &coords, uint32_t n, float &l, float &r) const
{
	l = r = 0.0f;
	const Tuples walked = applied_tuples(gid, coords, [&](float scalar, bool all, Bytes numbers_in, size_t numbers_at, DeltaStream &deltas) {
		int32_t v;
		if (all) {
			for (uint32_t i = 0; i < 2 * (n + 4); i++) { // the x deltas first
				if (!deltas.next(v))
					return false;
				if (i == n)
					l += (float)v * scalar;
				else if (i == n + 1)
					r += (float)v * scalar;
			}
			return true;
		}
		PointNumberStream numbers;
		(void)numbers.open(numbers_in, numbers_at); // (the walk checked them)
		while (numbers.got < numbers.count) {
			uint16_t number = 0;
			if (!numbers.next(number) || !deltas.next(v))
				return false;
			if (number == n)
				l += (float)v * scalar;
			else if (number == n + 1)
				r += (float)v * scalar;
		}
		for (uint32_t i = 0; i < numbers.count; i++) // the y deltas
			if (!deltas.next(v))
				return false;
		return true;
	});
	return walked == Tuples::None ? Face::kGvarAdvanceNone : walked == Tuples::Applied ? Face::kGvarAdvanceDelta : Face::kGvarAdvanceMalformed;
}

// ---- glyf ------------------------------------------------------------------------------
std::optional<Bytes> Face::glyph_data(uint16_t gid) const
{
	if (loca_.empty() || glyf_.empty() || gid == 0xFFFF || (size_t)gid + 1 >= loca_entries_)
		return std::nullopt;
	size_t a, b;
	if (loca_long_) {
		a = loca_.u32((size_t)gid * 4);
		b = loca_.u32((size_t)gid * 4 + 4);
	} else {
		a = (size_t)loca_.u16((size_t)gid * 2) * 2;
		b = (size_t)loca_.u16((size_t)gid * 2 + 2) * 2;
	}
	if (a >= b || b > glyf_.size())
		return std::nullopt;
	return glyf_.sub(a, b - a);
}

namespace {

// 2x3 affine of a composite component; f32 like ttf-parser's Transform
struct Affine {
	float a = 1.f, b = 0.f, c = 0.f, d = 1.f, e = 0.f, f = 0.f;
	bool identity() const { return a == 1.f && b == 0.f && c == 0.f && d == 1.f && e == 0.f && f == 0.f; }
	// parent.then(child): Transform::combine(parent, child)
	Affine then(const Affine &k) const
	{
		Affine r;
		r.a = a * k.a + c * k.b;
		r.b = b * k.a + d * k.b;
		r.c = a * k.c + c * k.d;
		r.d = b * k.c + d * k.d;
		r.e = a * k.e + c * k.f + e;
		r.f = b * k.e + d * k.f + f;
		return r;
	}
	void map(float &x, float &y) const
	{
		const float tx = x, ty = y;
		x = a * tx + c * ty + e;
		y = b * tx + d * ty + f;
	}
};

// Turns TrueType contour points into move/line/quad callbacks (ttf-parser glyf.rs Builder).  B: the sink — the
// OutlineBuilder interface (virtual calls), or a concrete recorder whose calls inline (the recording path of the device
// front-end spends as long in the sink as in the walk: 0.8 of 1.75 us per glyph).
template <class B> class ContourEmitter {
public:
	ContourEmitter(B &out, const Affine &t) : out_(out), t_(t), plain_(t.identity()) {}
	// a simple glyph of n_points in n_contours is about to be walked / has been walked: at most one command per point
	// plus, per contour, its close and up to two closing curves (a quad carries 4 floats)
	// (a sink with kRawCursor hands out two store cursors for that many commands; they live HERE, in an object that
	// never leaves walk()'s frame: byte stores through a cursor kept in the sink — which the recursive walk holds by
	// reference — would force the compiler to reload both cursors after every store)
	void begin(uint32_t n_points, uint32_t n_contours)
	{
		if constexpr (B::kRawCursor)
			out_.open((size_t)n_points + 3u * n_contours, 4u * ((size_t)n_points + 3u * n_contours), kp_, cp_);
	}
	void end()
	{
		if constexpr (B::kRawCursor)
			out_.shut(kp_, cp_);
	}

	void point(float x, float y, bool on_curve, bool last_of_contour)
	{
		if (!start_) {
			if (on_curve) {
				start_ = P{x, y};
				move(x, y);
			} else if (lead_off_) {
				const P m = mid(*lead_off_, P{x, y});
				start_ = m;
				pending_off_ = P{x, y};
				move(m.x, m.y);
			} else {
				lead_off_ = P{x, y};
			}
		} else if (pending_off_) {
			const P c = *pending_off_;
			if (on_curve) {
				pending_off_.reset();
				quad(c, P{x, y});
			} else {
				pending_off_ = P{x, y};
				quad(c, mid(c, P{x, y}));
			}
		} else if (on_curve) {
			line(x, y);
		} else {
			pending_off_ = P{x, y};
		}
		if (last_of_contour)
			finish();
	}

private:
	struct P {
		float x, y;
	};
	static P mid(P a, P b) { return P{a.x + 0.5f * (b.x - a.x), a.y + 0.5f * (b.y - a.y)}; } // lerp(.., 0.5)

	void finish()
	{
		if (lead_off_ && pending_off_) {
			const P c = *pending_off_;
			pending_off_.reset();
			quad(c, mid(c, *lead_off_));
		}
		if (start_ && lead_off_)
			quad(*lead_off_, *start_);
		else if (start_ && pending_off_)
			quad(*pending_off_, *start_);
		else if (start_)
			line(start_->x, start_->y);
		start_.reset();
		lead_off_.reset();
		pending_off_.reset();
		if constexpr (B::kRawCursor)
			*kp_++ = 4;
		else
			out_.close();
	}
	void move(float x, float y)
	{
		if (!plain_)
			t_.map(x, y);
		if constexpr (B::kRawCursor) {
			*kp_++ = 0;
			cp_[0] = x, cp_[1] = y;
			cp_ += 2;
		} else {
			out_.move_to(x, y);
		}
	}
	void line(float x, float y)
	{
		if (!plain_)
			t_.map(x, y);
		if constexpr (B::kRawCursor) {
			*kp_++ = 1;
			cp_[0] = x, cp_[1] = y;
			cp_ += 2;
		} else {
			out_.line_to(x, y);
		}
	}
	void quad(P c, P p)
	{
		if (!plain_) {
			t_.map(c.x, c.y);
			t_.map(p.x, p.y);
		}
		if constexpr (B::kRawCursor) {
			*kp_++ = 2;
			cp_[0] = c.x, cp_[1] = c.y, cp_[2] = p.x, cp_[3] = p.y;
			cp_ += 4;
		} else {
			out_.quad_to(c.x, c.y, p.x, p.y);
		}
	}

	B &out_;
	Affine t_;
	bool plain_;
	std::optional<P> start_, lead_off_, pending_off_;
	uint8_t *kp_ = nullptr; // kRawCursor: where the next kind byte / the next coordinates go
	float *cp_ = nullptr;
};

constexpr int kMaxComponentDepth = kGlyfMaxComponentDepth; // (glyf_table_limits.h)

enum : uint8_t { ON_CURVE = 0x01, X_SHORT = 0x02, Y_SHORT = 0x04, REPEAT = 0x08, X_SAME_POS = 0x10, Y_SAME_POS = 0x20 };

// simple glyph body (after numberOfContours + bbox); false = malformed (ttf-parser -> None)
// (E: ContourEmitter, or the point collector of the gvar walk)
template <class E> bool walk_simple(Bytes body, uint16_t n_contours, E &em)
{
	if (!body.has(0, (size_t)n_contours * 2))
		return false;
	const uint16_t last_end = body.u16((size_t)(n_contours - 1) * 2);
	if (last_end == 0xFFFF)
		return false;
	const uint32_t n_points = (uint32_t)last_end + 1;
	if (n_points == 1)
		return true; // a lone point yields nothing
	size_t cur = (size_t)n_contours * 2;
	if (!body.has(cur, 2))
		return false;
	cur += 2 + body.u16(cur); // instructions
	if (cur > body.size())
		return false;
	// pass 1: size of the flag / x / y arrays
	const size_t flags_at = cur;
	size_t xs = 0, ys = 0;
	for (uint32_t left = n_points; left;) {
		if (!body.has(cur, 1))
			return false;
		const uint8_t fl = body.u8(cur++);
		uint32_t run = 1;
		if (fl & REPEAT) {
			if (!body.has(cur, 1))
				return false;
			run += body.u8(cur++);
		}
		if (run > left)
			return false;
		xs += (fl & X_SHORT) ? run : ((fl & X_SAME_POS) ? 0 : 2 * run);
		ys += (fl & Y_SHORT) ? run : ((fl & Y_SAME_POS) ? 0 : 2 * run);
		left -= run;
	}
	const size_t x_at = cur, y_at = x_at + xs, y_end = y_at + ys;
	if (y_end > body.size())
		return false;
	// pass 2: decode
	size_t fp = flags_at, xp = x_at, yp = y_at;
	uint8_t fl = 0;
	uint32_t run_left = 0;
	int16_t x = 0, y = 0;
	uint32_t contour = 1, in_contour_left = body.u16(0); // EndpointsIter
	em.begin(n_points, n_contours);
	for (uint32_t i = 0; i < n_points; i++) {
		bool last;
		if (in_contour_left == 0) {
			if (contour < n_contours) {
				const uint16_t end = body.u16((size_t)contour * 2), prev = body.u16((size_t)(contour - 1) * 2);
				const uint16_t span = end > prev ? (uint16_t)(end - prev) : 0;
				in_contour_left = span ? span - 1u : 0u;
			}
			contour++;
			last = true;
		} else {
			in_contour_left--;
			last = false;
		}
		if (run_left == 0) {
			fl = fp < x_at ? body.u8(fp++) : 0;
			if (fl & REPEAT)
				run_left = fp < x_at ? body.u8(fp++) : 0;
		} else {
			run_left--;
		}
		int16_t dx = 0, dy = 0;
		if (fl & X_SHORT) {
			const int v = xp < y_at ? body.u8(xp++) : 0;
			dx = (int16_t)((fl & X_SAME_POS) ? v : -v);
		} else if (!(fl & X_SAME_POS) && xp + 2 <= y_at) {
			dx = body.i16(xp);
			xp += 2;
		}
		if (fl & Y_SHORT) {
			const int v = yp < y_end ? body.u8(yp++) : 0;
			dy = (int16_t)((fl & Y_SAME_POS) ? v : -v);
		} else if (!(fl & Y_SAME_POS) && yp + 2 <= y_end) {
			dy = body.i16(yp);
			yp += 2;
		}
		x = (int16_t)(uint16_t)((uint16_t)x + (uint16_t)dx); // wrapping
		y = (int16_t)(uint16_t)((uint16_t)y + (uint16_t)dy);
		em.point((float)x, (float)y, (fl & ON_CURVE) != 0, last);
	}
	em.end();
	return true;
}

// The gvar walk's (GvarWalker, which reads every composite twice: once to count its records, once to follow them): one component
// record of a composite's body at p, by the rules of GlyfWalker::walk's loop — its flags, its glyph id and its transform; p moves
// behind it.  false: the record leaves the entry (ttf-parser's iterator ends there).
inline bool read_component(Bytes body, size_t &p, uint16_t &flags, uint16_t &child, Affine &k)
{
	if (!body.has(p, 4))
		return false;
	flags = body.u16(p), child = body.u16(p + 2);
	p += 4;
	if (flags & 0x0002) { // ARGS_ARE_XY_VALUES
		if (flags & 0x0001) {
			if (!body.has(p, 4))
				return false;
			k.e = (float)body.i16(p);
			k.f = (float)body.i16(p + 2);
			p += 4;
		} else {
			if (!body.has(p, 2))
				return false;
			k.e = (float)(int8_t)body.u8(p);
			k.f = (float)(int8_t)body.u8(p + 1);
			p += 2;
		}
	} // anchor-point arguments are not consumed by ttf-parser 0.25 (parity unpinned)
	auto f2dot14 = [&](size_t at) { return (float)body.i16(at) / 16384.0f; };
	if (flags & 0x0080) {
		if (!body.has(p, 8))
			return false;
		k.a = f2dot14(p);
		k.b = f2dot14(p + 2);
		k.c = f2dot14(p + 4);
		k.d = f2dot14(p + 6);
		p += 8;
	} else if (flags & 0x0040) {
		if (!body.has(p, 4))
			return false;
		k.a = f2dot14(p);
		k.d = f2dot14(p + 2);
		p += 4;
	} else if (flags & 0x0008) {
		if (!body.has(p, 2))
			return false;
		k.a = k.d = f2dot14(p);
		p += 2;
	}
	return true;
}

} // namespace

// PARTS: the sink does not take callbacks but every simple glyph as it stands (B::part): the device decodes it
template <class B, bool PARTS> struct GlyfWalker {
	const Face &face;
	B &out;

	bool walk(Bytes glyph, int depth, const Affine &t)
	{
		if (depth >= kMaxComponentDepth || !glyph.has(0, 2))
			return false;
		const int16_t n_contours = glyph.i16(0);
		const Bytes body = glyph.from(10);
		if (n_contours > 0) {
			if (glyph.size() < 10)
				return false;
			if constexpr (PARTS) {
				return out.part(body, (uint16_t)n_contours, t.a, t.b, t.c, t.d, t.e, t.f, t.identity());
			} else {
				ContourEmitter<B> em(out, t);
				return walk_simple(body, (uint16_t)n_contours, em);
			}
		}
		if (n_contours == 0 || glyph.size() < 10)
			return n_contours == 0;
		// composite
		size_t p = 0;
		for (;;) {
			if (!body.has(p, 4))
				break;
			const uint16_t flags = body.u16(p), child = body.u16(p + 2);
			p += 4;
			Affine k;
			if (flags & 0x0002) { // ARGS_ARE_XY_VALUES
				if (flags & 0x0001) {
					if (!body.has(p, 4))
						break;
					k.e = (float)body.i16(p);
					k.f = (float)body.i16(p + 2);
					p += 4;
				} else {
					if (!body.has(p, 2))
						break;
					k.e = (float)(int8_t)body.u8(p);
					k.f = (float)(int8_t)body.u8(p + 1);
					p += 2;
				}
			} // anchor-point arguments are not consumed by ttf-parser 0.25 (parity unpinned)
			auto f2dot14 = [&](size_t at) { return (float)body.i16(at) / 16384.0f; };
			if (flags & 0x0080) {
				if (!body.has(p, 8))
					break;
				k.a = f2dot14(p);
				k.b = f2dot14(p + 2);
				k.c = f2dot14(p + 4);
				k.d = f2dot14(p + 6);
				p += 8;
			} else if (flags & 0x0040) {
				if (!body.has(p, 4))
					break;
				k.a = f2dot14(p);
				k.d = f2dot14(p + 2);
				p += 4;
			} else if (flags & 0x0008) {
				if (!body.has(p, 2))
					break;
				k.a = k.d = f2dot14(p);
				p += 2;
			}
			if (auto cd = face.glyph_data(child))
				if (!walk(*cd, depth + 1, t.then(k)))
					return false;
			if (!(flags & 0x0020)) // MORE_COMPONENTS
				break;
		}
		return true;
	}
};

namespace {
// the gvar walk's sinks: the callbacks of an OutlineBuilder, and the packed recorder
struct GvarCallbacks {
	static constexpr bool kRawCursor = false;
	OutlineBuilder &to;
	void move_to(float x, float y) { to.move_to(x, y); }
	void line_to(float x, float y) { to.line_to(x, y); }
	void quad_to(float x1, float y1, float x, float y) { to.quad_to(x1, y1, x, y); }
	void close() { to.close(); }
};
// walk_simple's sink of the gvar walk: the entry's points as they stand, for G5
struct PointCollector {
	std::vector<int16_t> x, y;
	std::vector<uint8_t> on_curve, last_of_contour;
	void begin(uint32_t n_points, uint32_t)
	{
		x.reserve(n_points), y.reserve(n_points), on_curve.reserve(n_points), last_of_contour.reserve(n_points);
	}
	void point(float px, float py, bool on, bool last)
	{
		x.push_back((int16_t)px), y.push_back((int16_t)py); // (whole numbers of i16 range: walk_simple made them of such)
		on_curve.push_back(on), last_of_contour.push_back(last);
	}
	void end() {}
};
} // namespace

// The walk of a face placed by `gvar` (G5, G6 of ttf_face.hpp): GlyfWalker's, glyph id by glyph id, with every entry's points
// moved by the sums GvarTable::accumulate has for it before the static walk's emitter and transforms see them.
// B: a sink type of the gvar walk's own (GvarCallbacks, GvarCursorSink below), so that the static walk's emitter remains the
// instantiation with one caller that it was.
template <class B> struct GvarWalker {
	const Face &face;
	const GvarTable &gvar;
	B &out;

	bool walk(uint16_t gid, int depth, const Affine &t)
	{
		const auto entry = face.glyph_data(gid);
		if (!entry)
			return depth != 0; // (a component without an entry is passed over, as in GlyfWalker)
		const Bytes glyph = *entry;
		if (depth >= kMaxComponentDepth || !glyph.has(0, 2))
			return false;
		const int16_t n_contours = glyph.i16(0);
		const Bytes body = glyph.from(10);
		std::vector<float> acc;
		if (n_contours > 0) {
			if (glyph.size() < 10)
				return false;
			PointCollector pc;
			if (!walk_simple(body, (uint16_t)n_contours, pc))
				return false;
			if (pc.x.empty())
				return true; // a lone point yields nothing
			const uint32_t n = (uint32_t)pc.x.size();
			if (!gvar.accumulate(gid, face.coords(), GvarPoints{n, pc.x.data(), pc.y.data(), pc.last_of_contour.data()}, acc))
				return false;
			ContourEmitter<B> em(out, t);
			em.begin(n, (uint16_t)n_contours);
			for (uint32_t i = 0; i < n; i++)
				em.point((float)pc.x[i] + acc[(size_t)2 * i], (float)pc.y[i] + acc[(size_t)2 * i + 1], pc.on_curve[i] != 0, pc.last_of_contour[i] != 0);
			em.end();
			return true;
		}
		if (n_contours == 0 || glyph.size() < 10)
			return n_contours == 0;
		// composite: one point per record the static walk reads
		uint32_t n_records = 0;
		for (size_t p = 0;;) {
			uint16_t flags, child;
			Affine k;
			if (!read_component(body, p, flags, child, k))
				break;
			n_records++;
			if (!(flags & 0x0020))
				break;
		}
		if (!gvar.accumulate(gid, face.coords(), GvarPoints{n_records}, acc))
			return false;
		uint32_t record = 0;
		for (size_t p = 0;; record++) {
			uint16_t flags, child;
			Affine k;
			if (!read_component(body, p, flags, child, k))
				break;
			k.e += acc[(size_t)2 * record];
			k.f += acc[(size_t)2 * record + 1];
			if (!walk(child, depth + 1, t.then(k)))
				return false;
			if (!(flags & 0x0020)) // MORE_COMPONENTS
				break;
		}
		return true;
	}
};

// G7: the points of the glyph id's own entry
bool Face::own_point_count(uint16_t gid, uint32_t &n) const
{
	n = 0;
	const auto entry = glyph_data(gid);
	if (!entry)
		return true; // no entry: no point, and still the four phantom ones
	const Bytes glyph = *entry;
	if (!glyph.has(0, 2))
		return false;
	const int16_t n_contours = glyph.i16(0);
	if (n_contours == 0)
		return true;
	if (glyph.size() < 10)
		return false;
	const Bytes body = glyph.from(10);
	if (n_contours > 0) {
		if (!body.has(0, (size_t)n_contours * 2))
			return false;
		const uint16_t last_end = body.u16((size_t)(n_contours - 1) * 2);
		if (last_end == 0xFFFF)
			return false;
		n = (uint32_t)last_end + 1;
		return true;
	}
	for (size_t p = 0;;) { // composite: one point per record the static walk reads
		uint16_t flags, child;
		Affine k;
		if (!read_component(body, p, flags, child, k))
			break;
		n++;
		if (!(flags & 0x0020))
			break;
	}
	return true;
}

uint8_t Face::gvar_advance_delta(uint16_t gid, float &d) const
{
	d = 0.0f;
	uint32_t n;
	if (!gvar_)
		return kGvarAdvanceNone;
	if (!own_point_count(gid, n))
		return kGvarAdvanceMalformed;
	float l, r;
	const uint8_t state = gvar_->phantom_sums(gid, coords_, n, l, r);
	if (state == kGvarAdvanceDelta)
		d = r - l;
	return state;
}

bool Face::outline_glyph(uint16_t gid, OutlineBuilder &builder) const
{
	if (!has_glyf_outlines() && cff_) // ttf-parser: glyf first, then cff
		return cff_->outline(gid, builder);
	if (gvar_) {
		GvarCallbacks sink{builder};
		GvarWalker<GvarCallbacks> w{*this, *gvar_, sink};
		return w.walk(gid, 0, Affine{});
	}
	const auto g = glyph_data(gid);
	if (!g)
		return false;
	GlyfWalker<OutlineBuilder, false> w{*this, builder};
	return w.walk(*g, 0, Affine{});
}

namespace {
// the callbacks in the compact upload form of vgsdf_outlines_packed: a kind byte per command + the coordinates it carries
struct PackedSink {
	std::vector<uint8_t> &kinds;
	std::vector<float> &coords;
	void move_to(float x, float y)
	{
		kinds.push_back(0);
		coords.push_back(x);
		coords.push_back(y);
	}
	void line_to(float x, float y)
	{
		kinds.push_back(1);
		coords.push_back(x);
		coords.push_back(y);
	}
	void quad_to(float x1, float y1, float x, float y)
	{
		kinds.push_back(2);
		coords.push_back(x1);
		coords.push_back(y1);
		coords.push_back(x);
		coords.push_back(y);
	}
	void close() { kinds.push_back(4); }
};
// The glyf walk's recorder: it announces every simple glyph's size first, room for its commands is made once (open),
// the emitter stores kind bytes and coordinates through two cursors of its own instead of three to five push_backs per
// command, shut() trims to what was written (2973 glyphs of Noto Sans: 30 -> 16 ns per command).
struct PackedCursorSink {
	static constexpr bool kRawCursor = true;
	std::vector<uint8_t> &kinds;
	std::vector<float> &coords;
	void open(size_t cmds, size_t floats, uint8_t *&kp, float *&cp)
	{
		const size_t k0 = kinds.size(), c0 = coords.size();
		// (batches are addressed with 32-bit offsets: a composite that fans one glyph out to gigabytes of commands is an error,
		// not a wrapped offset)
		if (k0 + cmds > (1ull << 30) || c0 + floats > (1ull << 30))
			throw std::length_error("glyph outlines: more than 2^30 commands in one batch (composite fan-out)");
		kinds.resize(k0 + cmds);
		coords.resize(c0 + floats);
		kp = kinds.data() + k0;
		cp = coords.data() + c0;
	}
	void shut(const uint8_t *kp, const float *cp)
	{
		kinds.resize((size_t)(kp - kinds.data()));
		coords.resize((size_t)(cp - coords.data()));
	}
};
struct GvarCursorSink : PackedCursorSink {}; // (the gvar walk's: GvarWalker)
// (CFF charstrings go through the OutlineBuilder interface)
struct PackedSinkVirtual final : OutlineBuilder {
	PackedSink s;
	explicit PackedSinkVirtual(PackedSink p) : s(p) {}
	void move_to(float x, float y) override { s.move_to(x, y); }
	void line_to(float x, float y) override { s.line_to(x, y); }
	void quad_to(float x1, float y1, float x, float y) override { s.quad_to(x1, y1, x, y); }
	void curve_to(float x1, float y1, float x2, float y2, float x, float y) override
	{
		s.kinds.push_back(3);
		for (float v : {x1, y1, x2, y2, x, y})
			s.coords.push_back(v);
	}
	void close() override { s.close(); }
};
} // namespace

namespace {
// Sink of the parts walk: what walk_simple checks BEFORE it touches the flag / coordinate arrays is checked here, with
// the same outcome (false: ttf-parser returns None, the walk of a composite stops); the arrays themselves are copied
// as they stand and checked where they are decoded (a mismatch there fails the batch: vgsdf.h, VGSDF_E_GLYF).
// what a simple glyph's entry says about itself before its arrays are looked at: shared by the sinks of the parts walk
struct PartShape {
	enum Kind { Fail, Nothing, Part }; // Fail: ttf-parser returns None here; Nothing: a lone point, no part, the walk goes on
	size_t cur = 0, ends = 0, arrays = 0; // cur: first byte behind the instructions; ends / arrays: bytes to copy (0 when !fits)
	uint32_t n_points = 0;
	bool fits = false;
	Kind measure(Bytes body, uint16_t n_contours)
	{
		if (!body.has(0, (size_t)n_contours * 2))
			return Fail;
		const uint16_t last_end = body.u16((size_t)(n_contours - 1) * 2);
		if (last_end == 0xFFFF)
			return Fail;
		n_points = (uint32_t)last_end + 1;
		if (n_points == 1)
			return Nothing; // a lone point yields nothing
		cur = (size_t)n_contours * 2;
		if (!body.has(cur, 2))
			return Fail;
		cur += 2 + body.u16(cur); // instructions: not needed on the device
		if (cur > body.size())
			return Fail;
		// (an entry longer than the device's decoder takes is not copied — one damaged `loca` entry could otherwise make every
		// glyph that names it carry megabytes: without its arrays the part fails there and the batch goes to the host's reader)
		constexpr size_t kMaxEntry = kGlyfMaxEntry; // (glyf_table_limits.h)
		fits = (size_t)n_contours * 2 + (body.size() - cur) <= kMaxEntry;
		ends = fits ? (size_t)n_contours * 2 : 0;
		arrays = fits ? body.size() - cur : 0;
		return Part;
	}
};
struct PartsSink {
	std::vector<GlyfPart> &parts;
	std::vector<uint8_t> &bytes;
	uint32_t &slots;
	bool *overflow;
	// A batch of parts is addressed with 32-bit offsets (vgsdf_glyf_part); a composite copies its simple glyphs once per
	// LEAF of its tree, so a small font can ask for gigabytes here (one 32 KB glyph named by 140 000 components).  Past
	// these bounds nothing more is recorded and the walk stops: the caller drops the glyf form for the batch.
	static constexpr uint64_t kMaxBatchSlots = 1ull << 26, kMaxBatchParts = 1ull << 22;
	static uint64_t max_batch_bytes()
	{
		static const uint64_t v = [] {
			const char *e = std::getenv("VG_GLYF_PARTS_LIMIT"); // (test switch: a small bound sends ordinary fonts down the fallback)
			return e ? std::max<uint64_t>(1024, std::strtoull(e, nullptr, 10)) : (1ull << 26);
		}();
		return v;
	}
	bool part(Bytes body, uint16_t n_contours, float a, float b, float c, float d, float e, float f, bool plain)
	{
		PartShape sh;
		if (const PartShape::Kind k = sh.measure(body, n_contours); k != PartShape::Part)
			return k == PartShape::Nothing;
		const size_t cur = sh.cur, ends = sh.ends, arrays = sh.arrays;
		const uint32_t n_points = sh.n_points;
		const bool fits = sh.fits;
		if ((uint64_t)bytes.size() + ends + arrays + 4 > max_batch_bytes() || (uint64_t)slots + n_points + 2ull * n_contours > kMaxBatchSlots ||
		    parts.size() >= kMaxBatchParts) {
			if (overflow)
				*overflow = true;
			return false;
		}
		GlyfPart p;
		p.byte_off = (uint32_t)bytes.size(); // (a multiple of 4: padded below)
		p.byte_len = (uint32_t)(ends + arrays);
		p.cmd_at = slots;
		// callbacks of a contour of L points: at most one per point, at most two from Builder::finish (the closing curves of a
		// contour that begins AND ends off the curve — whose first point then emitted nothing) and close(): L + 2 in every case
		p.cmd_cap = n_points + 2u * n_contours;
		p.n_contours = n_contours;
		p.plain = plain ? 1u : 0u;
		p.a = a, p.b = b, p.c = c, p.d = d, p.e = e, p.f = f;
		const size_t at = bytes.size(), padded = ((size_t)p.byte_len + 3) & ~(size_t)3;
		bytes.resize(at + padded); // (zero padding)
		if (fits) {
			std::memcpy(bytes.data() + at, body.data(), ends);
			std::memcpy(bytes.data() + at + ends, body.data() + cur, arrays);
		}
		slots += p.cmd_cap;
		parts.push_back(p);
		return true;
	}
};
} // namespace

bool Face::glyph_parts(uint16_t gid, std::vector<GlyfPart> &parts, std::vector<uint8_t> &bytes, uint32_t &slots, bool *overflow) const
{
	const auto g = has_glyf_form() ? glyph_data(gid) : std::nullopt;
	if (!g)
		return false;
	PartsSink sink{parts, bytes, slots, overflow};
	GlyfWalker<PartsSink, true> w{*this, sink};
	return w.walk(*g, 0, Affine{});
}

namespace {
// Sink of the resident table's walk: PartsSink's checks (PartShape), but the arrays of a simple glyph are stored once —
// entries are told apart by where they lie in the font (a damaged `loca` may make many glyph ids name one entry)
struct ResidentSink {
	ResidentTable &t;
	std::map<std::pair<const uint8_t *, size_t>, uint32_t> &stored; // (entry body, its length) -> byte_off
	uint32_t slots = 0; // of the glyph being walked
	bool overflow = false;
	bool part(Bytes body, uint16_t n_contours, float a, float b, float c, float d, float e, float f, bool plain)
	{
		PartShape sh;
		if (const PartShape::Kind k = sh.measure(body, n_contours); k != PartShape::Part)
			return k == PartShape::Nothing;
		GlyfPart p;
		p.byte_len = (uint32_t)(sh.ends + sh.arrays);
		p.cmd_at = slots;
		p.cmd_cap = sh.n_points + 2u * n_contours; // (PartsSink::part)
		p.n_contours = n_contours;
		p.plain = plain ? 1u : 0u;
		p.a = a, p.b = b, p.c = c, p.d = d, p.e = e, p.f = f;
		if ((uint64_t)slots + p.cmd_cap > ResidentTable::kMaxGlyphSlots || t.leaves.size() >= ResidentTable::kMaxLeaves) {
			overflow = true;
			return false;
		}
		const auto key = std::make_pair(body.data(), body.size());
		if (auto it = stored.find(key); it != stored.end()) {
			p.byte_off = it->second;
		} else {
			const size_t at = t.bytes.size(), padded = ((size_t)p.byte_len + 3) & ~(size_t)3;
			if ((uint64_t)at + padded > ResidentTable::kMaxBytes) {
				overflow = true;
				return false;
			}
			p.byte_off = (uint32_t)at;
			t.bytes.resize(at + padded); // (zero padding)
			if (sh.fits) {
				std::memcpy(t.bytes.data() + at, body.data(), sh.ends);
				std::memcpy(t.bytes.data() + at + sh.ends, body.data() + sh.cur, sh.arrays);
			}
			stored.emplace(key, p.byte_off);
		}
		slots += p.cmd_cap;
		t.leaves.push_back(p);
		return true;
	}
};
} // namespace

// serials of the tables a renderer keeps device copies of: one sequence for both kinds, so a key names one table
static uint64_t next_table_serial()
{
	static std::atomic<uint64_t> next_serial{1};
	return next_serial.fetch_add(1);
}

const ResidentTable &Face::resident_table() const
{
	ResidentCell &cell = *resident_;
	std::call_once(cell.once, [&] {
		ResidentTable &t = cell.table;
		if (!has_glyf_form())
			return;
		std::map<std::pair<const uint8_t *, size_t>, uint32_t> stored;
		const uint32_t n = num_glyphs_;
		t.leaf_off.assign(1, 0);
		t.slot_off.assign(1, 0);
		uint64_t slot_sum = 0;
		for (uint32_t gid = 0; gid < n; gid++) {
			ResidentSink sink{t, stored};
			if (const auto g = glyph_data((uint16_t)gid)) {
				GlyfWalker<ResidentSink, true> w{*this, sink};
				(void)w.walk(*g, 0, Affine{});
			}
			slot_sum += sink.slots;
			if (sink.overflow || slot_sum > kResidentMaxSlotSum) {
				t = ResidentTable{};
				return;
			}
			t.leaf_off.push_back((uint32_t)t.leaves.size());
			t.slot_off.push_back((uint32_t)slot_sum);
		}
		t.serial = resident_serial();
		t.ok = true;
	});
	return cell.table;
}

uint64_t Face::resident_serial() const
{
	ResidentCell &cell = *resident_;
	std::call_once(cell.serial_once, [&] { cell.serial = next_table_serial(); });
	return cell.serial;
}

FontTables Face::font_tables() const
{
	FontTables t;
	if (!has_glyf_form() || loca_.size() > 0xFFFFFFFFu || glyf_.size() > 0xFFFFFFFFu)
		return t;
	t.loca = loca_.data(), t.n_loca_bytes = (uint32_t)loca_.size();
	t.glyf = glyf_.data(), t.n_glyf_bytes = (uint32_t)glyf_.size();
	t.num_glyphs = num_glyphs_, t.loca_entries = (uint32_t)loca_entries_, t.loca_long = loca_long_ ? 1u : 0u;
	t.ok = true;
	return t;
}

GvarTables Face::gvar_tables() const
{
	GvarTables t;
	if (!placed_by_gvar() || loca_.size() > 0xFFFFFFFFu || glyf_.size() > 0xFFFFFFFFu || gvar_->table().size() > 0xFFFFFFFFu)
		return t;
	t.tables.loca = loca_.data(), t.tables.n_loca_bytes = (uint32_t)loca_.size();
	t.tables.glyf = glyf_.data(), t.tables.n_glyf_bytes = (uint32_t)glyf_.size();
	t.tables.num_glyphs = num_glyphs_, t.tables.loca_entries = (uint32_t)loca_entries_, t.tables.loca_long = loca_long_ ? 1u : 0u;
	t.tables.ok = true;
	t.gvar = gvar_->table().data(), t.gvar_len = (uint32_t)gvar_->table().size();
	t.n_axes = (uint32_t)coords().size(), t.coords = coords().data();
	t.shared_tuple_count = gvar_->shared_tuple_count(), t.glyph_count = gvar_->glyph_count();
	t.ok = true;
	return t;
}

namespace {
// counts what a glyph's callbacks would add to a CommandTable; past the bounds it ends the walk (a composite can fan a few
// kilobytes out to billions of callbacks)
struct PastCommandBounds {};
struct CountingBuilder final : OutlineBuilder {
	uint64_t cmds = 0, floats = 0, max_cmds = 0;
	void add(uint64_t n_floats)
	{
		cmds++, floats += n_floats;
		if (cmds > max_cmds || floats > CommandTable::kMaxFloats)
			throw PastCommandBounds{};
	}
	void move_to(float, float) override { add(2); }
	void line_to(float, float) override { add(2); }
	void quad_to(float, float, float, float) override { add(4); }
	void curve_to(float, float, float, float, float, float) override { add(6); }
	void close() override { add(0); }
};
} // namespace

const CommandTable &Face::command_table() const
{
	CommandCell &cell = *commands_;
	std::call_once(cell.once, [&] {
		CommandTable &t = cell.table;
		const uint32_t n = num_glyphs_;
		CountingBuilder count;
		count.max_cmds = (CommandTable::kMaxStoreBytes - 4 * ((uint64_t)n + 1)) / CommandTable::kStoreBytesPerCmd;
		try {
			for (uint32_t gid = 0; gid < n; gid++)
				(void)outline_glyph((uint16_t)gid, count);
		} catch (const PastCommandBounds &) {
			return;
		}
		t.kinds.reserve((size_t)count.cmds);
		t.coords.reserve((size_t)count.floats);
		t.cmd_off.assign(1, 0);
		t.dat_off.assign(1, 0);
		for (uint32_t gid = 0; gid < n; gid++) {
			(void)outline_glyph_packed((uint16_t)gid, t.kinds, t.coords);
			t.cmd_off.push_back((uint32_t)t.kinds.size());
			t.dat_off.push_back((uint32_t)t.coords.size());
		}
		t.serial = command_serial();
		t.ok = true;
	});
	return cell.table;
}

uint64_t Face::command_serial() const
{
	CommandCell &cell = *commands_;
	std::call_once(cell.serial_once, [&] { cell.serial = next_table_serial(); });
	return cell.serial;
}

const CharstringTable &Face::charstring_table() const
{
	CommandCell &cell = *commands_;
	std::call_once(cell.charstrings_once, [&] {
		CharstringTable &t = cell.charstrings;
		if (has_glyf_outlines() || !cff_ || cff_->is_cff2())
			return;
		if (!cff_->charstring_table(num_glyphs_, t)) {
			t = CharstringTable{};
			return;
		}
		t.serial = command_serial();
		t.ok = true;
	});
	return cell.charstrings;
}

const CharstringTable &Face::charstring2_table() const
{
	CommandCell &cell = *commands_;
	std::call_once(cell.charstrings2_once, [&] {
		CharstringTable &t = cell.charstrings2;
		if (has_glyf_outlines() || !cff_ || !cff_->is_cff2())
			return;
		if (!cff_->charstring_table(num_glyphs_, t)) {
			t = CharstringTable{};
			return;
		}
		t.serial = command_serial();
		t.ok = true;
	});
	return cell.charstrings2;
}

bool Face::outline_glyph_packed(uint16_t gid, std::vector<uint8_t> &kinds, std::vector<float> &coords) const
{
	PackedSink sink{kinds, coords};
	if (!has_glyf_outlines() && cff_) {
		PackedSinkVirtual v(sink);
		return cff_->outline(gid, v);
	}
	if (gvar_) {
		GvarCursorSink cursor{{kinds, coords}};
		GvarWalker<GvarCursorSink> w{*this, *gvar_, cursor};
		return w.walk(gid, 0, Affine{});
	}
	const auto g = glyph_data(gid);
	if (!g)
		return false;
	PackedCursorSink cursor{kinds, coords};
	GlyfWalker<PackedCursorSink, false> w{*this, cursor};
	return w.walk(*g, 0, Affine{});
}

} // namespace vg
