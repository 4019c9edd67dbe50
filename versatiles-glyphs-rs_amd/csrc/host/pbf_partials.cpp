// Partial PBFs of one block (the ranks of a glyph-level shard, the lanes of a split block) joined into the block's file.
#include "font_manager.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace vg {

std::vector<uint8_t> merge_pbf_partials(const std::vector<std::pair<const uint8_t *, size_t>> &parts)
{
	struct G {
		uint32_t id;
		const uint8_t *p; // the glyph message's payload
		size_t n;
	};
	auto varint = [](const uint8_t *&p, const uint8_t *end, uint64_t &v) {
		v = 0;
		for (int sh = 0; p < end && sh < 64; sh += 7) {
			const uint8_t b = *p++;
			v |= (uint64_t)(b & 0x7F) << sh;
			if (!(b & 0x80))
				return true;
		}
		return false;
	};
	std::string name, range;
	bool have = false;
	std::vector<G> glyphs;
	for (const auto &part : parts) {
		const uint8_t *p = part.first, *end = p + part.second;
		uint64_t len;
		if (p == end || *p++ != 0x0A || !varint(p, end, len) || len != (uint64_t)(end - p))
			throw std::runtime_error("merge_pbf_partials: not a glyphs PBF with one fontstack");
		std::string nm, rg;
		while (p < end) {
			const uint8_t tag = *p++;
			if (!varint(p, end, len) || len > (uint64_t)(end - p))
				throw std::runtime_error("merge_pbf_partials: truncated field");
			if (tag == 0x0A) {
				nm.assign((const char *)p, (size_t)len);
			} else if (tag == 0x12) {
				rg.assign((const char *)p, (size_t)len);
			} else if (tag == 0x1A) {
				const uint8_t *q = p, *qe = p + len;
				uint64_t id;
				if (q == qe || *q++ != 0x08 || !varint(q, qe, id))
					throw std::runtime_error("merge_pbf_partials: glyph without id");
				glyphs.push_back(G{(uint32_t)id, p, (size_t)len});
			} else {
				throw std::runtime_error("merge_pbf_partials: unexpected field");
			}
			p += len;
		}
		if (have && (nm != name || rg != range))
			throw std::runtime_error("merge_pbf_partials: parts of different blocks (" + name + "/" + range + " vs " + nm + "/" + rg + ")");
		name = nm, range = rg, have = true;
	}
	std::stable_sort(glyphs.begin(), glyphs.end(), [](const G &a, const G &b) { return a.id < b.id; });
	auto vsize = [](uint64_t v) {
		size_t n = 1;
		for (; v >= 0x80; v >>= 7)
			n++;
		return n;
	};
	auto put = [](std::vector<uint8_t> &o, uint64_t v) {
		for (; v >= 0x80; v >>= 7)
			o.push_back((uint8_t)(v | 0x80));
		o.push_back((uint8_t)v);
	};
	size_t stack = 1 + vsize(name.size()) + name.size() + 1 + vsize(range.size()) + range.size();
	for (const G &g : glyphs)
		stack += 1 + vsize(g.n) + g.n;
	std::vector<uint8_t> out;
	out.reserve(1 + vsize(stack) + stack);
	out.push_back(0x0A);
	put(out, stack);
	out.push_back(0x0A);
	put(out, name.size());
	out.insert(out.end(), name.begin(), name.end());
	out.push_back(0x12);
	put(out, range.size());
	out.insert(out.end(), range.begin(), range.end());
	for (const G &g : glyphs) {
		out.push_back(0x1A);
		put(out, g.n);
		out.insert(out.end(), g.p, g.p + g.n);
	}
	return out;
}

// The same for parts that hold CONSECUTIVE runs of a block's code points, in order (the split blocks of the hybrid lane plan):
// the entries of a part are already in ascending id and stay together, so the block's file is its header followed by the
// parts' entry regions as they are — three or four copies instead of a walk over every glyph message.  The first ids of the
// parts must ascend (checked); anything unexpected goes to merge_pbf_partials.
bool plan_pbf_concat(const std::vector<std::pair<const uint8_t *, size_t>> &parts, std::vector<uint8_t> &head,
                     std::vector<std::pair<const uint8_t *, size_t>> &pieces)
{
	auto varint = [](const uint8_t *&p, const uint8_t *end, uint64_t &v) {
		v = 0;
		for (int sh = 0; p < end && sh < 64; sh += 7) {
			const uint8_t b = *p++;
			v |= (uint64_t)(b & 0x7F) << sh;
			if (!(b & 0x80))
				return true;
		}
		return false;
	};
	head.clear();
	pieces.clear();
	const uint8_t *fields = nullptr; // name + range fields of the first part
	size_t fields_n = 0;
	uint64_t last_first_id = 0;
	bool any = false;
	for (const auto &part : parts) {
		const uint8_t *p = part.first, *end = p + part.second;
		uint64_t len;
		if (p == end || *p++ != 0x0A || !varint(p, end, len) || len != (uint64_t)(end - p))
			return false;
		const uint8_t *f0 = p;
		for (int k = 0; k < 2; k++) { // 0x0A name, 0x12 range (fontstack.rs:9-25: in tag order)
			if (p == end || *p++ != (k ? 0x12 : 0x0A) || !varint(p, end, len) || len > (uint64_t)(end - p))
				return false;
			p += len;
		}
		if (!fields) {
			fields = f0;
			fields_n = (size_t)(p - f0);
		} else if ((size_t)(p - f0) != fields_n || std::memcmp(f0, fields, fields_n) != 0) {
			return false; // (parts of different blocks: merge_pbf_partials says so)
		}
		if (p == end)
			continue; // a part without glyphs
		const uint8_t *q = p;
		uint64_t glen, id;
		if (*q++ != 0x1A || !varint(q, end, glen) || q == end || *q++ != 0x08 || !varint(q, end, id) || (any && id <= last_first_id))
			return false;
		last_first_id = id;
		any = true;
		pieces.emplace_back(p, (size_t)(end - p));
	}
	if (!fields)
		return false;
	size_t stack = fields_n;
	for (const auto &r : pieces)
		stack += r.second;
	head.push_back(0x0A);
	for (uint64_t v = stack;; v >>= 7) {
		if (v < 0x80) {
			head.push_back((uint8_t)v);
			break;
		}
		head.push_back((uint8_t)(v | 0x80));
	}
	head.insert(head.end(), fields, fields + fields_n);
	pieces.insert(pieces.begin(), std::make_pair((const uint8_t *)head.data(), head.size()));
	return true;
}

std::vector<uint8_t> concat_pbf_partials(const std::vector<std::pair<const uint8_t *, size_t>> &parts)
{
	std::vector<uint8_t> head, out;
	std::vector<std::pair<const uint8_t *, size_t>> pieces;
	if (!plan_pbf_concat(parts, head, pieces))
		return merge_pbf_partials(parts);
	size_t total = 0;
	for (const auto &pc : pieces)
		total += pc.second;
	out.reserve(total);
	for (const auto &pc : pieces)
		out.insert(out.end(), pc.first, pc.first + pc.second);
	return out;
}

} // namespace vg
