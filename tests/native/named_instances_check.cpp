// Runs the readers behind vg_manager_add_font_named_instances (csrc/host/ttf_face.hpp: read_variation_axes with the instance
// records and their postScriptNameID, named_instance_ps_names over the `name` table) over the font files named on the command
// line, and over EVERY TRUNCATION of each file's fvar and name table: the table is moved to the end of a copy of the file that is
// allocated to end exactly where the table is cut, and the directory states the cut length, so a read past the cut leaves the
// allocation.  Compiled with -fsanitize=address,undefined together with ttf_face.cpp and cff.cpp
// (tests/test_named_instances_sanitized.py): the readers must stay inside the file.
// One line per file: "<path>: ok <axes> <instances> <cuts>|<family>|<ps name>|..." (the names of the whole file) | "no fvar".
// Exit 1: a result that breaks its own rules (an instance without one coordinate per axis, not one name per instance).
#include "cff.hpp"
#include "ttf_face.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

namespace {
uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

// both readers over data[0, len); false: a result that breaks its rules
bool read(const uint8_t *data, size_t len, std::vector<vg::VariationAxis> &axes, std::vector<vg::NamedInstance> &instances, std::string &family,
          std::vector<std::string> &names, bool &has_fvar)
{
	has_fvar = vg::read_variation_axes(data, len, axes, &instances);
	if (!has_fvar)
		return true;
	for (const vg::NamedInstance &ni : instances)
		if (ni.coords.size() != axes.size())
			return false;
	if (vg::named_instance_ps_names(data, len, instances, family, names) && names.size() != instances.size())
		return false;
	return true;
}
} // namespace

int main(int argc, char **argv)
{
	int bad = 0;
	for (int a = 1; a < argc; a++) {
		std::ifstream in(argv[a], std::ios::binary);
		const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		std::vector<vg::VariationAxis> axes;
		std::vector<vg::NamedInstance> instances;
		std::string family;
		std::vector<std::string> names;
		bool has_fvar = false, ok = read(data.data(), data.size(), axes, instances, family, names, has_fvar);
		if (!has_fvar) {
			std::printf("%s: no fvar\n", argv[a]);
			continue;
		}
		size_t cuts = 0;
		const uint32_t n_tables = data.size() >= 12 ? ((uint32_t)data[4] << 8 | data[5]) : 0;
		for (uint32_t t = 0; t < n_tables && 12 + 16 * (size_t)(t + 1) <= data.size(); t++) {
			const size_t rec = 12 + 16 * (size_t)t;
			if (std::memcmp(&data[rec], "fvar", 4) != 0 && std::memcmp(&data[rec], "name", 4) != 0)
				continue;
			const size_t off = be32(&data[rec + 8]), length = be32(&data[rec + 12]);
			if (off > data.size() || length > data.size() - off)
				continue;
			for (size_t cut = 0; cut <= length; cut++, cuts++) {
				const size_t n = data.size() + cut;
				std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
				std::memcpy(copy.get(), data.data(), data.size());
				std::memcpy(copy.get() + data.size(), data.data() + off, cut);
				put32(copy.get() + rec + 8, (uint32_t)data.size());
				put32(copy.get() + rec + 12, (uint32_t)cut);
				std::vector<vg::VariationAxis> ax;
				std::vector<vg::NamedInstance> inst;
				std::string fam;
				std::vector<std::string> nm;
				bool any = false;
				ok = read(copy.get(), n, ax, inst, fam, nm, any) && ok;
				ok = ok && inst.size() <= instances.size(); // (a cut table offers no more than the whole one)
			}
		}
		std::printf("%s: %s %zu %zu %zu|%s", argv[a], ok ? "ok" : "BROKEN", axes.size(), instances.size(), cuts, family.c_str());
		for (const std::string &s : names)
			std::printf("|%s", s.c_str());
		std::printf("\n");
		bad += !ok;
	}
	return bad ? 1 : 0;
}
