// Runs the readers a face at a position adds (csrc/host/ttf_face.hpp: fvar axes and named instances, avar, Face::parse_at with
// its HVAR store, Face::glyph_hor_advance through the advance map and the ItemVariationData rows, Face::family_tables() with its
// variation part) over the font files named on the command line, each at three positions.  Compiled with
// -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp and run on edge tables and on truncated and damaged copies
// of them (tests/test_variation_tables_sanitized.py): the readers must stay inside the file.
// One line per file: "<path>: placed <axes> <instances> <regions> <checksum>" | "refused <why>" | "no fvar".  Exit 1: a
// description that breaks its own rules.
#include "cff.hpp"
#include "ttf_face.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
	int bad = 0;
	for (int a = 1; a < argc; a++) {
		std::ifstream in(argv[a], std::ios::binary);
		const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		std::vector<vg::VariationAxis> axes;
		std::vector<vg::NamedInstance> instances;
		if (!vg::read_variation_axes(data.data(), data.size(), axes, &instances)) {
			std::printf("%s: no fvar\n", argv[a]);
			continue;
		}
		if (axes.size() > 64)
			axes.resize(64);
		uint32_t sum = 0;
		size_t regions = 0;
		std::string why;
		bool placed = false, ok = true;
		for (int pos = 0; pos < 3; pos++) {
			std::vector<int16_t> coords;
			for (const vg::VariationAxis &ax : axes)
				coords.push_back(vg::normalize_axis_value(ax, pos == 0 ? ax.max : pos == 1 ? (ax.def + ax.max) / 2 : ax.min));
			vg::apply_avar(data.data(), data.size(), coords);
			const auto face = vg::Face::parse_at(data.data(), data.size(), coords, &why);
			if (!face)
				break;
			placed = true;
			regions = face->hvar_region_scalars().size();
			for (uint32_t g = 0; g < (uint32_t)face->number_of_glyphs() + 2u && g <= 0xFFFFu; g++)
				sum = sum * 31 + face->glyph_hor_advance((uint16_t)g).value_or(0xFFFF);
			const vg::FamilyTables &t = face->family_tables();
			if (t.ok && t.hvar) {
				ok = ok && t.hvar >= data.data() && t.hvar + t.hvar_len <= data.data() + data.size() && (uint64_t)t.hvar_store + 8 <= t.hvar_len &&
				     t.hvar_map < t.hvar_len && t.region_scalars.size() == regions;
				for (uint32_t i = 0; ok && i < t.hvar_len; i++)
					sum = sum * 31 + t.hvar[i];
			}
		}
		if (!placed)
			std::printf("%s: refused %s\n", argv[a], why.c_str());
		else
			std::printf("%s: %s %zu %zu %zu %08x\n", argv[a], ok ? "placed" : "BROKEN", axes.size(), instances.size(), regions, sum);
		bad += !ok;
	}
	return bad ? 1 : 0;
}
