// Builds Face::font_tables() (csrc/host/ttf_face.hpp: the description of a face's `loca` and `glyf` for the device's table builder)
// for the font files named on the command line, checks what vgsdf_font_create_tables would check, reads every byte the description
// names and every loca entry it counts, and builds the table the description stands in for (Face::resident_table) from the same
// bytes.  Compiled with -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run on the fixtures, on edge fonts
// and on damaged copies (tests/test_font_tables_sanitized.py): the builder and the reader under it must stay inside the file.
// One line per file: "<path>: described <num_glyphs> <loca_entries> <checksum> <leaves or refused>" | "no glyf" | "not a font".
// Exit 1: a description that breaks its own rules.
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
		const vg::FontTables t = face->font_tables();
		if (!t.ok) {
			std::printf("%s: no glyf\n", argv[a]);
			bad += face->has_glyf_outlines();
			continue;
		}
		const uint8_t *lo = data.data(), *hi = data.data() + data.size();
		bool ok = t.num_glyphs <= 0xFFFF && t.loca_long <= 1 && t.n_loca_bytes && t.n_glyf_bytes && t.loca >= lo && t.loca + t.n_loca_bytes <= hi &&
		          t.glyf >= lo && t.glyf + t.n_glyf_bytes <= hi && (uint64_t)t.loca_entries * (t.loca_long ? 4u : 2u) <= t.n_loca_bytes &&
		          t.loca_entries <= (t.num_glyphs == 0xFFFF ? 0xFFFFu : t.num_glyphs + 1u);
		uint32_t sum = 0;
		for (uint32_t i = 0; ok && i < t.loca_entries * (t.loca_long ? 4u : 2u); i++)
			sum = sum * 31 + t.loca[i];
		for (uint32_t i = 0; ok && i < t.n_glyf_bytes; i++)
			sum = sum * 31 + t.glyf[i];
		const vg::ResidentTable &r = face->resident_table();
		if (r.ok)
			std::printf("%s: %s %u %u %08x %zu\n", argv[a], ok ? "described" : "BROKEN", t.num_glyphs, t.loca_entries, sum, r.leaves.size());
		else
			std::printf("%s: %s %u %u %08x refused\n", argv[a], ok ? "described" : "BROKEN", t.num_glyphs, t.loca_entries, sum);
		bad += !ok;
	}
	return bad ? 1 : 0;
}
