// Runs the `gvar` reader (csrc/host/gvar.hpp and the rules G1 to G6 of ttf_face.hpp: Face::parse_at of a glyf face, outline_glyph
// and outline_glyph_packed of every glyph id, command_table()) over the font files named on the command line, each at the
// positions given in front of them.  Compiled with -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run on
// the hand-written tables of tests/gvar_instances_kit.py, on truncated ones and on damaged copies
// (tests/test_gvar_tables_sanitized.py): the reader must stay inside the file.
// Usage: gvar_tables_check <n positions> <coordinate>... <file>...   (a coordinate is given to every axis)
// One line per file: "<path>: placed <axes> <glyph ids> <glyph ids that return false> <checksum>" | "refused <why>" | "no fvar".
// Exit 1: the two outline calls, or the table and the calls, disagree.
#include "ttf_face.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

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
		uint32_t sum = 0, n_false = 0, n_glyphs = 0;
		std::string why;
		bool placed = false, ok = true;
		for (const int16_t pos : positions) {
			const std::vector<int16_t> coords(axes.size(), pos);
			const auto face = vg::Face::parse_at(data.data(), data.size(), coords, &why);
			if (!face)
				break;
			placed = true;
			ok = ok && !face->has_glyf_form() && !face->font_tables().ok && !face->resident_table().ok;
			n_glyphs = face->number_of_glyphs();
			const vg::CommandTable &t = face->command_table();
			for (uint32_t g = 0; g < n_glyphs + 2u && g <= 0xFFFFu; g++) {
				std::vector<uint8_t> kinds;
				std::vector<float> floats;
				const bool drew = face->outline_glyph_packed((uint16_t)g, kinds, floats);
				n_false += !drew;
				if (t.ok && g < n_glyphs) {
					const size_t c0 = t.cmd_off[g], c1 = t.cmd_off[g + 1], d0 = t.dat_off[g], d1 = t.dat_off[g + 1];
					ok = ok && c1 - c0 == kinds.size() && d1 - d0 == floats.size() &&
					     (kinds.empty() || std::memcmp(kinds.data(), t.kinds.data() + c0, kinds.size()) == 0) &&
					     (floats.empty() || std::memcmp(floats.data(), t.coords.data() + d0, floats.size() * 4) == 0);
				}
				for (const uint8_t k : kinds)
					sum = sum * 31 + k;
				for (const float v : floats) {
					uint32_t bits;
					std::memcpy(&bits, &v, 4);
					sum = sum * 31 + bits;
				}
			}
		}
		if (!placed)
			std::printf("%s: refused %s\n", argv[a], why.c_str());
		else
			std::printf("%s: %s %zu %u %u %08x\n", argv[a], ok ? "placed" : "BROKEN", axes.size(), n_glyphs, n_false, sum);
		bad += !ok;
	}
	return bad ? 1 : 0;
}
