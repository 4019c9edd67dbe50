// gvar.hpp — `gvar`: the deltas a `glyf` face's points take at a position of the design space (Face::parse_at).  The rules are
// G1 to G5 of ttf_face.hpp, written from the OpenType specification; where it leaves the f32 order open the order stated
// there is the definition.  PARITY WITH THE CRATE UNPINNED, as for the rest of the variation code (cff.hpp).
// Implemented in ttf_face.cpp: that file and cff.cpp are the whole reader for whoever compiles it on its own.
#pragma once
#include <cstdint>
#include <optional>
#include <vector>

#include "ttf_face.hpp"

namespace vg {

// One glyf entry's points as G5 / G6 see them.  A simple glyph: its n points' original coordinates and, per point, whether it
// is the last of its contour (the static walk's own contour iterator says so).  A composite: one point per component record,
// x / y / last_of_contour left empty (nothing is inferred).  The 4 phantom points follow in both cases.
struct GvarPoints {
	uint32_t n = 0; // without the phantom points
	const int16_t *x = nullptr, *y = nullptr;
	const uint8_t *last_of_contour = nullptr;
};

class GvarTable {
public:
	// nullopt: not readable — a version other than 1.0, an axisCount other than n_axes, or a header, shared tuples or offset
	// array that leave the table
	static std::optional<GvarTable> parse(Bytes table, uint32_t n_axes);
	// G1 to G5 for one entry: acc (2 floats per point, x then y, the phantom points included: 2 * (pts.n + 4)) is set to the
	// sums of the glyph id's tuples at coords (as many as the table has axes).  false: malformed data — acc is not to be used.
	bool accumulate(uint16_t glyph_id, const std::vector<int16_t> &coords, const GvarPoints &pts, std::vector<float> &acc) const;
	// G7 for one entry of n points: l and r, the sums of the x deltas of points n and n + 1 over the glyph id's tuples at coords,
	// streamed (no per-point storage; every applied tuple's numbers and deltas are walked to their end, so that malformed means
	// what it means to accumulate).  Face::kGvarAdvanceNone: no variation data (l = r = 0), kGvarAdvanceDelta, or
	// kGvarAdvanceMalformed (l and r are not to be used).
	uint8_t phantom_sums(uint16_t glyph_id, const std::vector<int16_t> &coords, uint32_t n, float &l, float &r) const;

	Bytes table() const { return table_; }
	uint32_t axis_count() const { return axis_count_; }
	uint32_t shared_tuple_count() const { return shared_count_; }
	uint32_t glyph_count() const { return glyph_count_; }

private:
	// G1 to G4, the one walk over a glyph id's tuples that accumulate and phantom_sums both are (ttf_face.cpp states the visitor)
	enum class Tuples { None, Applied, Malformed };
	template <class Visit> Tuples applied_tuples(uint16_t glyph_id, const std::vector<int16_t> &coords, Visit &&visit) const;

	Bytes table_;
	uint32_t axis_count_ = 0, shared_count_ = 0, shared_at_ = 0, glyph_count_ = 0, data_at_ = 0;
	bool long_offsets_ = false;
};

} // namespace vg
