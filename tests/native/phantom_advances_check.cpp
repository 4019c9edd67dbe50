// Runs rule G7 of ttf_face.hpp (advances of a placed glyf face from gvar's phantom points: Face::parse_at with gvar_advances,
// gvar_advance_delta and glyph_hor_advance of every glyph id, hor_advances) over the font files named on the command line, each at
// the positions given in front of them.  Compiled with -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run
// on the hand-written faces of tests/phantom_advances_kit.py, on every truncation of their gvar and on damaged copies
// (tests/test_phantom_advances_sanitized.py): the streaming walk must stay inside the file.
// Usage: phantom_advances_check <n positions> <coordinate>... <file>...   (a coordinate is given to every axis)
// One line per file: "<path>: placed <axes> <glyph ids> <deltas> <malformed> <advances moved> <checksum>" (the three counts over
// all positions) | "refused <why>" | "no fvar".
// Exit 1: an advance that is not the rule's over the delta and the advance of the same face placed without the option, or a face
// that follows G7 although it should not (or the reverse); or a glyph id for which GvarTable::phantom_sums and GvarTable::accumulate
// (the same glyph id, coordinates and point count, no contours given) disagree: one malformed and the other not, or l / r not the
// 32 bits of acc[2 * n] / acc[2 * (n + 1)].  Bit equality is the rule's own: nothing is inferred without contours, ascending numbers
// write no point twice within a tuple, and both add (float)v * scalar for the same tuples in the same order.
#include "gvar.hpp"
#include "ttf_face.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

// G7's point count of the glyph id's own entry, restated over the tables the face hands to the device (Face's own is private):
// false: the entry is malformed.  This copy is validated where it is used: sums_agree's last line requires that the state and
// delta the face itself computes (with its own count) are those of the sums taken with this one, so a drift here fails the run.
static bool own_point_count(const vg::FontTables &t, uint32_t gid, uint32_t &n)
{
	n = 0;
	if (t.n_loca_bytes == 0 || t.n_glyf_bytes == 0 || gid == 0xFFFFu || gid + 1 >= t.loca_entries)
		return true;
	const vg::Bytes loca(t.loca, t.n_loca_bytes);
	const size_t a = t.loca_long ? loca.u32((size_t)gid * 4) : (size_t)loca.u16((size_t)gid * 2) * 2;
	const size_t b = t.loca_long ? loca.u32((size_t)gid * 4 + 4) : (size_t)loca.u16((size_t)gid * 2 + 2) * 2;
	if (a >= b || b > t.n_glyf_bytes)
		return true;
	const vg::Bytes glyph(t.glyf + a, b - a);
	if (glyph.size() < 2)
		return false;
	const int16_t n_contours = glyph.i16(0);
	if (n_contours == 0)
		return true;
	if (glyph.size() < 10)
		return false;
	const vg::Bytes body = glyph.from(10);
	if (n_contours > 0) {
		if (!body.has(0, (size_t)n_contours * 2) || body.u16((size_t)(n_contours - 1) * 2) == 0xFFFF)
			return false;
		n = (uint32_t)body.u16((size_t)(n_contours - 1) * 2) + 1;
		return true;
	}
	for (size_t p = 0; body.has(p, 4);) { // one point per component record: flags and child, arguments if x and y, transform
		const uint16_t flags = body.u16(p);
		const size_t args = (flags & 0x0002) ? ((flags & 0x0001) ? 4 : 2) : 0;
		const size_t form = (flags & 0x0080) ? 8 : (flags & 0x0040) ? 4 : (flags & 0x0008) ? 2 : 0;
		if (!body.has(p + 4, args) || !body.has(p + 4 + args, form))
			break;
		p += 4 + args + form;
		n++;
		if (!(flags & 0x0020))
			break;
	}
	return true;
}

static uint32_t bits_of(float f)
{
	uint32_t u;
	std::memcpy(&u, &f, 4);
	return u;
}

// G7 held against G1 to G5 directly: the advance pass and the outline's accumulation (no contours given: nothing is inferred)
// refuse the same glyph ids, and where both succeed l and r are bit for bit the x sums of points n and n + 1
static bool sums_agree(const vg::Face &face, const vg::GvarTable &gvar, const vg::GvarTables &t, uint16_t gid)
{
	uint32_t n;
	if (!own_point_count(t.tables, gid, n))
		return true; // (a malformed entry: gvar is not asked)
	const std::vector<int16_t> coords(t.coords, t.coords + t.n_axes);
	float l, r, d;
	std::vector<float> acc;
	const uint8_t state = gvar.phantom_sums(gid, coords, n, l, r);
	const bool outline = gvar.accumulate(gid, coords, vg::GvarPoints{n}, acc);
	if (outline != (state != vg::Face::kGvarAdvanceMalformed))
		return false;
	if (outline && (acc.size() != (size_t)2 * (n + 4) || bits_of(l) != bits_of(acc[(size_t)2 * n]) || bits_of(r) != bits_of(acc[(size_t)2 * (n + 1)])))
		return false;
	// (and the count above is the face's: its own delta is that of these sums)
	return face.gvar_advance_delta(gid, d) == state && (state != vg::Face::kGvarAdvanceDelta || bits_of(d) == bits_of(r - l));
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const int n_pos = std::atoi(argv[1]);
	if (n_pos < 1 || argc < 2 + n_pos)
		return 2;
	std::vector<int16_t> positions;
	for (int i = 0; i < n_pos; i++)
		positions.push_back((int16_t)std::atoi(argv[2 + i]));
	int bad = 0;
	for (int a = 2 + n_pos; a < argc; a++) {
		std::ifstream in(argv[a], std::ios::binary);
		const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		std::vector<vg::VariationAxis> axes;
		if (!vg::read_variation_axes(data.data(), data.size(), axes)) {
			std::printf("%s: no fvar\n", argv[a]);
			continue;
		}
		if (axes.size() > 64)
			axes.resize(64);
		uint32_t sum = 0, n_delta = 0, n_malformed = 0, n_moved = 0, n_glyphs = 0;
		std::string why;
		bool placed = false, ok = true;
		for (const int16_t pos : positions) {
			const std::vector<int16_t> coords(axes.size(), pos);
			const auto face = vg::Face::parse_at(data.data(), data.size(), coords, &why, true);
			const auto plain = vg::Face::parse_at(data.data(), data.size(), coords, &why);
			if (!face || !plain) {
				ok = ok && !face && !plain;
				break;
			}
			placed = true;
			ok = ok && !plain->advances_by_gvar() && (!face->advances_by_gvar() || face->placed_by_gvar());
			n_glyphs = face->number_of_glyphs();
			const std::vector<uint16_t> all = face->hor_advances(n_glyphs + 2u);
			const vg::GvarTables tables = face->gvar_tables();
			const auto gvar = tables.ok ? vg::GvarTable::parse(vg::Bytes(tables.gvar, tables.gvar_len), tables.n_axes) : std::nullopt;
			ok = ok && gvar.has_value() == face->placed_by_gvar();
			for (uint32_t g = 0; g < n_glyphs + 2u && g <= 0xFFFFu; g++) {
				ok = ok && (!gvar || sums_agree(*face, *gvar, tables, (uint16_t)g));
				float d = 0.0f;
				const uint8_t state = face->gvar_advance_delta((uint16_t)g, d);
				const auto got = face->glyph_hor_advance((uint16_t)g), stood = plain->glyph_hor_advance((uint16_t)g);
				ok = ok && all[g] == got.value_or(0);
				if (face->advances_by_gvar() && stood && state != vg::Face::kGvarAdvanceMalformed) {
					float want = (float)*stood;
					want += d + 0.5f;
					const bool none = !(want > -1.0f && want < 65536.0f);
					ok = ok && got.has_value() == !none && (none || *got == (uint16_t)(int32_t)want);
				} else {
					ok = ok && got == stood;
				}
				n_delta += state == vg::Face::kGvarAdvanceDelta;
				n_malformed += state == vg::Face::kGvarAdvanceMalformed;
				n_moved += got != stood;
				uint32_t bits;
				std::memcpy(&bits, &d, 4);
				sum = (sum * 31 + bits) * 31 + state;
				sum = sum * 31 + got.value_or(0xFFFF);
			}
		}
		if (!placed)
			std::printf("%s: refused %s\n", argv[a], why.c_str());
		else
			std::printf("%s: %s %zu %u %u %u %u %08x\n", argv[a], ok ? "placed" : "BROKEN", axes.size(), n_glyphs, n_delta, n_malformed, n_moved, sum);
		bad += !ok;
	}
	return bad ? 1 : 0;
}
