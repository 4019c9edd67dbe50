// Runs rule G7 of ttf_face.hpp (advances of a placed glyf face from gvar's phantom points: Face::parse_at with gvar_advances,
// gvar_advance_delta and glyph_hor_advance of every glyph id, hor_advances) over the font files named on the command line, each at
// the positions given in front of them.  Compiled with -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run
// on the hand-written faces of tests/phantom_advances_kit.py, on every truncation of their gvar and on damaged copies
// (tests/test_phantom_advances_sanitized.py): the streaming walk must stay inside the file.
// Usage: phantom_advances_check <n positions> <coordinate>... <file>...   (a coordinate is given to every axis)
// One line per file: "<path>: placed <axes> <glyph ids> <deltas> <malformed> <advances moved> <checksum>" (the three counts over
// all positions) | "refused <why>" | "no fvar".
// Exit 1: an advance that is not the rule's over the delta and the advance of the same face placed without the option, or a face
// that follows G7 although it should not (or the reverse).
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
			for (uint32_t g = 0; g < n_glyphs + 2u && g <= 0xFFFFu; g++) {
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
