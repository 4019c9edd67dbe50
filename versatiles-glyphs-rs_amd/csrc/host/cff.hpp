// cff.hpp — `CFF ` (version 1) outlines: the slice of ttf-parser's cff1 table (crate ttf-parser 0.25.1, a
// third-party dependency of the reference, not vendored under /root/reference) behind
//   Face::outline_glyph      /root/reference/src/render/renderer.rs:110
// for OpenType fonts whose outlines are Type 2 charstrings.  The charstring interpreter follows Adobe
// Technical Note #5177 ("The Type 2 Charstring Format") and #5176 (CFF); the crate's observable rules are
// kept: callbacks in f32 with one addition per coordinate in operand order, `close()` before every further
// `move_to` and at `endchar`, the optional width operand taken once, at most 48 operands and 10 nested
// subroutine calls, a glyph without any point yields no outline.
// No fixture of the reference holds CFF outlines: parity with the crate is UNPINNED here; the reader is
// checked against fontTools' charstring interpreter instead (tests/test_cff_outlines.py).
// `endchar` in its seac form (an accented character assembled from two glyphs of the standard encoding) draws the
// base glyph and then the accent at (adx, ady), each as a charstring of its own, through the font's charset.
// Not handled (-> no outline for that glyph): the arithmetic / storage operators of ESC (ttf-parser rejects them
// too), seac in CID-keyed fonts or with the Expert charsets.
//
// `CFF2` (variable fonts; the crate's cff2 table, used when the face has neither `glyf` nor a readable `CFF `): the
// same interpreter without width operand, `endchar` and `return` (operators 0, 2, 9, 11, 13, 14, 17 end the glyph), with
// up to 513 operands, 32-bit INDEX counts, one set of local subroutines (the first Font DICT whose Private DICT has
// one; FDSelect is not consulted) and the `vsindex` / `blend` operators.  The reference never sets variation
// coordinates (renderer.rs:103-110 uses the face as parsed), so every glyph is drawn at the default position of the
// design space: a region's factor is 1 where all its axes peak at 0 (or are malformed in one of the ways the crate
// maps to 1) and 0 otherwise, and `blend` adds delta * factor to its operands in f32, last region first.  Two
// rules of the crate that a reader written from the specification alone would not have: a face without `fvar` has
// NO coordinates, which makes every factor 1 (all deltas are added); and the scalars of ItemVariationData 0 are
// loaded before the first operator, so a table without a VariationStore yields no outline at all.
// PARITY UNPINNED like the rest of CFF, and more so: these rules are restated from the crate's documented behaviour
// without a fixture; the default-position outlines are checked against fontTools (tests/test_cff2_outlines.py).
//
// A face made by Face::parse_at carries coordinates other than 0 (the crate's set_variation): the factor of an axis of a
// region is then axis_factor below at the face's coordinate — 1 for a malformed or neutral axis, 0 at and outside the region's
// ends, else ONE f32 divide of the two differences, each converted to f32 first — and a region's factor the f32 product over
// the face's coordinates in axis order, 0 as soon as one factor is 0.  These rules (and those of `avar` and `HVAR` in
// ttf_face.hpp) are restated from the crate's set_variation / glyph_hor_advance as read, without the crate at hand: parity
// UNPINNED as well; outlines at a position are checked against fontTools (tests/test_variable_instances_host.py).
#pragma once
#include <cstdint>
#include <optional>
#include <vector>

#include "ttf_face.hpp"

namespace vg {

// Factor of one axis of a variation region at normalised coordinate `coord` (the crate's evaluate_axis; all values F2Dot14 as
// integers).  At coord 0 only 0 and 1 can come out: the interpolating branches need start < 0 < end with the peak off 0, which
// the second rule has already answered with 1.
float axis_factor(int16_t coord, int16_t start, int16_t peak, int16_t end);
// Factor of region `region` of a VariationRegionList (`list` from its axisCount; the caller has checked that its
// axisCount * regionCount records of 6 bytes lie inside) at `coords`: the product above.  The flat record index is kept in 16
// bits, as the crate computes it: a face with more coordinates than the list has axes reads on into the next region's records,
// and an index past 0xFFFF or past the records gives 0.
float variation_region_factor(Bytes list, uint32_t region, const std::vector<int16_t> &coords);

class CffTable {
public:
	static std::optional<CffTable> parse(Bytes table);
	// `CFF2`; coords = the face's normalised variation coordinates (F2Dot14; one per fvar axis, at most 64; all 0 for a face
	// made by Face::parse), none without `fvar`
	static std::optional<CffTable> parse2(Bytes table, const std::vector<int16_t> &coords);
	bool is_cff2() const { return cff2_; }
	uint32_t number_of_glyphs() const { return charstrings_.count; }
	// false = ttf-parser returns None (callbacks already delivered stay delivered)
	bool outline(uint16_t glyph_id, OutlineBuilder &builder) const;
	// The charstrings and subroutines of the face as the device's decoder takes them (CharstringTable of ttf_face.hpp), from the
	// tables parse() has located: every body copied once, every INDEX offset resolved and checked.  false (nothing of `out` is
	// to be used): an INDEX entry that does not ascend or leaves its data, or 256 Font DICTs in use AND a glyph without one
	// (Font DICTs past the 256 an FDSelect byte can name are left out; a glyph without Font DICT gets an empty set behind the font's own).
	// n_glyph_ids = the face's numGlyphs: glyph ids past the CharStrings INDEX get an empty charstring (no outline, as outline())
	// A CFF2 table: the one set of local subroutines parse2() picked (false past 65535 of them or of the global ones: the device's
	// description cannot state such a set), and every blend set with its ok flag and its factors as the reader uses them.
	bool charstring_table(uint32_t n_glyph_ids, CharstringTable &out) const;

private:
	struct Index {
		Bytes data;        // the whole INDEX
		uint32_t count = 0;
		uint8_t off_size = 1;
		size_t offsets_at = 0, data_at = 0; // byte positions inside `data`
		std::optional<Bytes> get(uint32_t i) const;
	};
	static bool parse_index(Bytes table, size_t at, Index &out, size_t &end, bool count32 = false);
	struct PrivateDict {
		Index local_subrs;
	};
	static bool parse_private(Bytes table, size_t offset, size_t size, PrivateDict &out);
	uint32_t fd_index_for(uint16_t glyph_id) const; // CID-keyed fonts: the glyph's Font DICT by FDSelect, 0xFFFFFFFF: none
	const Index *local_subrs_for(uint16_t glyph_id) const;
	// glyph of a code of Adobe's StandardEncoding (seac operands), through the charset; nullopt: none
	std::optional<uint16_t> standard_code_to_glyph(uint32_t code) const;

	Bytes table_;
	Index global_subrs_, charstrings_;
	bool cid_ = false;
	PrivateDict private_;              // name-keyed fonts
	std::vector<PrivateDict> fd_priv_; // CID-keyed fonts: one per font dict
	Bytes fd_select_;                  // CID-keyed fonts: FDSelect, from its format byte
	size_t charset_at_ = 0;            // Top DICT `charset`: 0 / 1 / 2 = ISOAdobe / Expert / ExpertSubset, else its offset
	// CFF2: per ItemVariationData subtable the factor of each of its regions at the face's position
	struct BlendSet {
		bool ok = false; // false: no such subtable, or more than 64 regions (the crate's limit)
		std::vector<float> scalars;
	};
	bool cff2_ = false;
	std::vector<BlendSet> blend_sets_;

	friend struct CharStringRun;
};

} // namespace vg
