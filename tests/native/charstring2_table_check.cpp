// Builds Face::charstring2_table() (csrc/host/ttf_face.hpp: the description of a `CFF2` face for the device's charstring decoder)
// for the font files named on the command line, checks what vgsdf_font_create_charstrings2 would check — every offset inside
// `bytes`, the blend sets inside the factors — and reads every byte and every factor the description names.  Compiled with
// -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run on a variable font and on copies of it damaged
// inside the `CFF2` table (tests/test_charstring2_table_sanitized.py): the parser under it must stay inside the file.
// One line per file: "<path>: described <glyph ids> <bytes> <sets> <checksum>" | "no description" | "not a font".  Exit 1: a
// description that breaks its own rules.
#include "cff.hpp"
#include "ttf_face.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

static bool ascends_inside(const std::vector<uint32_t> &off, size_t n_bytes)
{
	if (off.empty())
		return false;
	for (size_t i = 0; i + 1 < off.size(); i++)
		if (off[i + 1] < off[i])
			return false;
	return off.back() <= n_bytes;
}

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
		const vg::CharstringTable &t = face->charstring2_table();
		if (!t.ok) {
			std::printf("%s: no description\n", argv[a]);
			continue;
		}
		const size_t n = face->number_of_glyphs();
		bool ok = t.cff2 && t.bytes.size() % 4 == 0 && t.cs_off.size() == n + 1 && ascends_inside(t.cs_off, t.bytes.size()) &&
		          ascends_inside(t.gsubr_off, t.bytes.size()) && ascends_inside(t.lsubr_off, t.bytes.size()) && t.n_fds == 1 &&
		          t.lsubr_first.size() == 2 && t.lsubr_first[0] == 0 && t.lsubr_first[1] + 1 == t.lsubr_off.size() && t.fd_of.empty() &&
		          t.gsubr_off.size() - 1 <= 0xFFFFu && t.lsubr_off.size() - 1 <= 0xFFFFu && t.serial == face->command_serial() &&
		          t.set_off.size() == t.set_ok.size() + 1 && t.set_off[0] == 0 && ascends_inside(t.set_off, t.factors.size()) &&
		          t.set_off.back() == t.factors.size();
		for (size_t s = 0; ok && s < t.set_ok.size(); s++)
			ok = t.set_off[s + 1] - t.set_off[s] <= 64 && (t.set_ok[s] == 1 || (t.set_ok[s] == 0 && t.set_off[s + 1] == t.set_off[s]));
		uint32_t sum = 0;
		if (ok) {
			for (const std::vector<uint32_t> *off : {&t.cs_off, &t.gsubr_off, &t.lsubr_off})
				for (size_t i = 0; i + 1 < off->size(); i++)
					for (uint32_t p = (*off)[i]; p < (*off)[i + 1]; p++)
						sum = sum * 31 + t.bytes[p];
			for (float f : t.factors) {
				ok = ok && std::isfinite(f);
				sum = sum * 31 + (f != 0.0f);
			}
		}
		// (the command table of the same face: the reader the description stands in for walks the same bytes)
		const vg::CommandTable &c = face->command_table();
		ok = ok && (!c.ok || c.serial == t.serial);
		// the version 1 description is not there for a CFF2 face
		ok = ok && !face->charstring_table().ok;
		std::printf("%s: %s %zu %zu %zu %08x\n", argv[a], ok ? "described" : "BROKEN", n, t.bytes.size(), t.set_ok.size(), sum);
		bad += !ok;
	}
	return bad ? 1 : 0;
}
