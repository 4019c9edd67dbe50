// Builds Face::family_tables() (csrc/host/ttf_face.hpp: the description of a face's `cmap` and `hmtx` for the device's family-table
// kernels) for the font files named on the command line, checks what vgsdf_family_create_tables would check and reads every byte
// the description names, then walks every listed subtable the way the description's own regularity check did.  Compiled with
// -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run on the fixtures, on edge tables and on damaged copies
// (tests/test_family_tables_sanitized.py): the builder under it must stay inside the file.
// One line per file: "<path>: described <subtables> <cmap bytes> <checksum>" | "refused" | "not a font".  Exit 1: a description
// that breaks its own rules.
#include "cff.hpp"
#include "ttf_face.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

int main(int argc, char **argv)
{
	int bad = 0;
	for (int a = 1; a < argc; a++) {
		std::ifstream in(argv[a], std::ios::binary);
		const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		const auto face = vg::Face::parse(data.data(), data.size());
		if (!face) {
			std::printf("%s: not a font\n", argv[a]);
			continue;
		}
		const vg::FamilyTables &t = face->family_tables();
		// (the reader the description stands in for walks the same bytes, whatever the description says)
		uint32_t mapped = 0;
		for (uint32_t c : face->unicode_codepoints())
			mapped += face->glyph_index(c).has_value() && face->glyph_hor_advance(*face->glyph_index(c)).value_or(0) >= 0;
		if (!t.ok) {
			std::printf("%s: refused %u\n", argv[a], mapped);
			continue;
		}
		bool ok = t.subtable_off.size() == t.subtable_format.size() && t.subtable_off.size() <= 0xFFFF && t.units_per_em >= 16 &&
		          t.units_per_em <= 16384 && (t.cmap_len == 0 || t.cmap) && (t.hmtx_len == 0 || t.hmtx) &&
		          (t.cmap_len == 0 || (t.cmap >= data.data() && t.cmap + t.cmap_len <= data.data() + data.size())) &&
		          (t.hmtx_len == 0 || (t.hmtx >= data.data() && t.hmtx + t.hmtx_len <= data.data() + data.size()));
		uint32_t sum = 0;
		for (uint32_t i = 0; ok && i < t.cmap_len; i++)
			sum = sum * 31 + t.cmap[i];
		for (uint32_t i = 0; ok && i < t.hmtx_len; i++)
			sum = sum * 31 + t.hmtx[i];
		for (size_t s = 0; ok && s < t.subtable_off.size(); s++) {
			const uint16_t f = t.subtable_format[s];
			ok = t.subtable_off[s] < t.cmap_len && (f == 0 || f == 4 || f == 6 || f == 10 || f == 12 || f == 13) &&
			     (size_t)t.subtable_off[s] + 2 <= t.cmap_len &&
			     (uint16_t)((t.cmap[t.subtable_off[s]] << 8) | t.cmap[t.subtable_off[s] + 1]) == f;
		}
		std::printf("%s: %s %zu %u %08x %u\n", argv[a], ok ? "described" : "BROKEN", t.subtable_off.size(), t.cmap_len, sum, mapped);
		bad += !ok;
	}
	return bad ? 1 : 0;
}
