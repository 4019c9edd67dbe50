// ttf_face.hpp — the slice of ttf_parser::Face (crate ttf-parser 0.25.1, a third-party
// dependency of the reference, not vendored under /root/reference) that the render path
// calls:
//   Face::glyph_index        /root/reference/src/render/renderer.rs:106
//   Face::units_per_em       renderer.rs:107
//   Face::outline_glyph      renderer.rs:110   (glyf outlines -> OutlineBuilder callbacks)
//   Face::glyph_hor_advance  renderer.rs:115
//   cmap subtable walk       src/font/metadata.rs:105-117 (code point coverage)
// Static fonts: TrueType (`glyf`) outlines and `CFF ` (version 1) charstrings (cff.hpp); CFF2 / variable
// fonts are out of scope (none in the reference's testdata) and are refused at load time.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../glyf_table_limits.h"

namespace vg {

class CffTable;
class GvarTable;

// ttf_parser::OutlineBuilder — f32 font units
struct OutlineBuilder {
	virtual ~OutlineBuilder() = default;
	virtual void move_to(float x, float y) = 0;
	virtual void line_to(float x, float y) = 0;
	virtual void quad_to(float x1, float y1, float x, float y) = 0;
	virtual void curve_to(float x1, float y1, float x2, float y2, float x, float y) = 0;
	virtual void close() = 0;
	static constexpr bool kRawCursor = false; // (the glyf walk's packed recorder in ttf_face.cpp is the sink that has one)
};

// One simple glyph of a (possibly composite) glyph in the form the device's glyf decoder takes (vgsdf_glyf_part of
// include/vgsdf.h, field for field): the entry's end points + flag / coordinate arrays copied into a byte store, the
// component transform ttf-parser has accumulated, and the command slots the entry may fill.
struct GlyfPart {
	uint32_t byte_off, byte_len;
	uint32_t cmd_at, cmd_cap;
	uint32_t n_contours, plain;
	float a, b, c, d, e, f;
};

// A face's outlines in the form that stays on the device (vgsdf_font_desc of include/vgsdf.h): the leaves — simple glyphs
// with their accumulated transforms — of EVERY glyph id, and every simple glyph's arrays stored once however many
// composites name it.  A leaf's cmd_at counts from its glyph's first slot.
struct ResidentTable {
	bool ok = false;                // false: the face has no resident form (not glyf, or past the bounds below)
	uint64_t serial = 0;            // of the face, handed out when the table is built: what a renderer keys its device copy by
	std::vector<uint32_t> leaf_off; // [numGlyphs + 1]
	std::vector<uint32_t> slot_off; // [numGlyphs + 1] running sum of the glyphs' command slots (a host convenience: 64-bit safe below 2^32 by the bounds)
	std::vector<GlyfPart> leaves;
	std::vector<uint8_t> bytes;     // 4-aligned entries
	// bounds: more leaves than 2^22, a glyph of more than 2^26 slots, or a store past what 32-bit offsets address
	// (glyf_table_limits.h: the device's table builder refuses at the same bounds)
	static constexpr uint64_t kMaxLeaves = kResidentMaxLeaves, kMaxGlyphSlots = kResidentMaxGlyphSlots, kMaxBytes = kResidentMaxBytes;
};

// A face's outlines as the callbacks its reader delivers, glyph id by glyph id, in the arrays of the packed upload form
// (vgsdf_font_cmds_desc of include/vgsdf.h): the resident form of every face this reader can read, whatever table its
// outlines come from.  A glyph whose charstring or entry fails midway holds the callbacks delivered up to there.
struct CommandTable {
	bool ok = false;                // false: the store these commands make on the device (29 bytes each + 4 per glyph id), or their
	                                // coordinates, pass what 32-bit offsets address
	uint64_t serial = 0;            // of the table (never that of a ResidentTable): what a renderer keys its device copy by
	std::vector<uint32_t> cmd_off;  // [numGlyphs + 1] into kinds
	std::vector<uint32_t> dat_off;  // [numGlyphs + 1] into coords
	std::vector<uint8_t> kinds;
	std::vector<float> coords;
	static constexpr uint64_t kMaxStoreBytes = (1ull << 32) - 4, kStoreBytesPerCmd = 29, kMaxFloats = kMaxStoreBytes / 4;
};

// A `CFF ` (version 1) or `CFF2` face's charstrings for the device's decoder (vgsdf_font_charstrings_desc / _charstrings2_desc of
// include/vgsdf.h, array for array): every charstring and subroutine body copied once into `bytes`, the INDEX offsets resolved to
// ranges of it.  The store the device makes of it is the one CommandTable describes, so the two share the face's command serial.
struct CharstringTable {
	bool ok = false;                   // false: no outlines of the table's kind (Face::charstring_table: `CFF `, Face::charstring2_table:
	                                   // `CFF2`), or an INDEX the description cannot state
	uint64_t serial = 0;               // Face::command_serial()
	std::vector<uint8_t> bytes;        // padded to a multiple of 4
	std::vector<uint32_t> cs_off;      // [numGlyphs + 1]
	std::vector<uint32_t> gsubr_off;   // [global subroutines + 1]
	uint32_t n_fds = 1;
	std::vector<uint32_t> lsubr_first; // [n_fds + 1]
	std::vector<uint32_t> lsubr_off;   // [lsubr_first[n_fds] + 1]
	std::vector<uint8_t> fd_of;        // [numGlyphs], empty when n_fds == 1
	// CFF2 only: the blend sets, one per ItemVariationData of the variation store, with the reader's factors (at the face's
	// position: the default one unless the face was made by Face::parse_at)
	bool cff2 = false;
	std::vector<uint8_t> set_ok;       // [sets] 0: a charstring that selects the set ends there
	std::vector<uint32_t> set_off;     // [sets + 1] into factors
	std::vector<float> factors;
	// the same face but for the factors: every array the device's decoder is given equal, and as many factors
	bool same_face(const CharstringTable &o) const
	{
		return cff2 == o.cff2 && n_fds == o.n_fds && factors.size() == o.factors.size() && set_off == o.set_off && set_ok == o.set_ok &&
		       lsubr_first == o.lsubr_first && lsubr_off == o.lsubr_off && gsubr_off == o.gsubr_off && cs_off == o.cs_off && fd_of == o.fd_of &&
		       bytes == o.bytes;
	}
};

// A face's `cmap` and `hmtx` for the device's family-table kernels (vgsdf_face_tables of include/vgsdf.h, field for field): views of
// the two tables and where the unicode subtables are.  No code point is looked up.
struct FamilyTables {
	bool ok = false;                       // false: a format 4 subtable whose segments, or a format 12 / 13 subtable whose groups, are
	                                       // not regular (the device's bisection and the reader's enumeration could then disagree)
	const uint8_t *cmap = nullptr, *hmtx = nullptr; // views into the face's bytes
	uint32_t cmap_len = 0, hmtx_len = 0;
	uint16_t units_per_em = 0, num_glyphs = 0, num_hmetrics = 0;
	std::vector<uint32_t> subtable_off;    // into cmap: the encoding records, in the table's order, that are unicode and of format
	std::vector<uint16_t> subtable_format; // 0, 4, 6, 10, 12 or 13 (2, 8, 14 and unreadable ones map nothing and are left out)
	// a face at a position whose advances follow `HVAR` (vgsdf_face_variation of include/vgsdf.h, field for field); hvar is
	// nullptr for every other face.  Not ok as well (hvar_refused): an advance map of a format other than 0 and 1, or an
	// ItemVariationData with more word deltas than regions — the reader gives such glyphs their `hmtx` advance, the device is
	// not asked to
	bool hvar_refused = false;
	const uint8_t *hvar = nullptr;
	uint32_t hvar_len = 0, hvar_store = 0, hvar_map = 0; // offsets into hvar; hvar_map 0: no advance map
	std::vector<float> region_scalars; // the factor of every region of the store at the face's position
};

// What `fvar` offers (host only): its axes in user space, and its named instances
struct VariationAxis {
	char tag[4];
	float min, def, max;
};
struct NamedInstance {
	uint16_t name_id;
	std::vector<float> coords; // one per axis, user space
	uint16_t ps_name_id = 0xFFFF; // postScriptNameID of a record that has room for one (instanceSize >= 4 + 4 axes + 2); 0xFFFF: none
};
// false: no readable `fvar` (version 1.0, at least one axis, the axis records inside the table).  Instance records that
// leave the table are left out.
bool read_variation_axes(const uint8_t *data, size_t len, std::vector<VariationAxis> &axes, std::vector<NamedInstance> *instances = nullptr);
// The PostScript name a named instance is known by, from the file's `name` table (its records as Face::names() reads them, a
// later record of an id replacing an earlier one): the string of the record's postScriptNameID when that is not 0xFFFF and `name`
// has it; otherwise the variations PostScript name prefix (name id 25; absent or empty: the family name, id 1, without everything
// but ASCII letters and digits), "-", and the string of the record's subfamilyNameID (absent: empty) without its spaces.
// family: the file's name id 1 (absent: empty).  false: the file does not parse as a face.
bool named_instance_ps_names(const uint8_t *data, size_t len, const std::vector<NamedInstance> &instances, std::string &family,
                             std::vector<std::string> &ps_names);
// A user-space value of an axis as a normalised coordinate (F2Dot14), in f32: clamped to [min, max]; 0 at the default, else
// (v - def) / (def - min) below it and (v - def) / (max - def) above; clamped to [-1, 1], times 16384, truncated toward zero.
// (The crate's rule as read; whether it truncates or rounds is unpinned.)
int16_t normalize_axis_value(const VariationAxis &axis, float v);
// The file's `avar` (version 1.0 with as many segment maps as there are coordinates; anything else changes nothing) applied
// to normalised coordinates in place: per axis the piecewise-linear map over its records in i32 with rounding, truncating
// division; an empty map, or a result outside i16, leaves the value as it is.
void apply_avar(const uint8_t *data, size_t len, std::vector<int16_t> &coords);

// A `glyf` face's `loca` and `glyf` for the device's table builder (vgsdf_font_tables_desc of include/vgsdf.h, field for field):
// views of the two tables and the three numbers Face::glyph_data goes by.  No glyph is looked at.
struct FontTables {
	bool ok = false;                                // false: no glyf form (Face::has_glyf_form), or a table of 4 GiB or more
	const uint8_t *loca = nullptr, *glyf = nullptr; // views into the face's bytes
	uint32_t n_loca_bytes = 0, n_glyf_bytes = 0;
	uint32_t num_glyphs = 0, loca_entries = 0, loca_long = 0;
};

// A placed `glyf` face's tables for the device's gvar builder (vgsdf_font_gvar_desc of include/vgsdf.h): FontTables' views of
// loca and glyf (filled although the face has no glyf form: its entries are outlines only together with gvar), a view of the
// whole gvar, and the face's coordinates.  No glyph is looked at.
struct GvarTables {
	bool ok = false; // false: not a face placed by gvar (Face::placed_by_gvar), or a table of 4 GiB or more
	FontTables tables;
	const uint8_t *gvar = nullptr;
	uint32_t gvar_len = 0, n_axes = 0;
	const int16_t *coords = nullptr; // [n_axes]: the face's own, alive as long as the face
	// the header numbers, as GvarTable::parse read them
	uint32_t shared_tuple_count = 0, glyph_count = 0;
};

// Non-owning big-endian byte view with checked reads.
class Bytes {
public:
	Bytes() = default;
	Bytes(const uint8_t *p, size_t n) : p_(p), n_(n) {}
	size_t size() const { return n_; }
	bool empty() const { return n_ == 0; }
	const uint8_t *data() const { return p_; }
	bool has(size_t off, size_t len) const { return off <= n_ && len <= n_ - off; }
	uint8_t u8(size_t off) const { return p_[off]; }
	uint16_t u16(size_t off) const { return (uint16_t)((p_[off] << 8) | p_[off + 1]); }
	int16_t i16(size_t off) const { return (int16_t)u16(off); }
	uint32_t u32(size_t off) const
	{
		return ((uint32_t)p_[off] << 24) | ((uint32_t)p_[off + 1] << 16) | ((uint32_t)p_[off + 2] << 8) |
		       (uint32_t)p_[off + 3];
	}
	Bytes sub(size_t off, size_t len) const { return has(off, len) ? Bytes(p_ + off, len) : Bytes(); }
	Bytes from(size_t off) const { return off <= n_ ? Bytes(p_ + off, n_ - off) : Bytes(); }

private:
	const uint8_t *p_ = nullptr;
	size_t n_ = 0;
};

class Face {
public:
	// Face::parse(data, 0).  The bytes must outlive the Face.
	static std::optional<Face> parse(const uint8_t *data, size_t len);
	// (The rules of a position — normalisation, avar, region factors, HVAR — are the crate's set_variation / glyph_hor_advance as
	// read, without the crate at hand: PARITY UNPINNED, see cff.hpp.)
	// The same face AT A POSITION of its design space (the crate's set_variation for every axis): coords are final normalised
	// coordinates, F2Dot14, one per `fvar` axis (at most 64 are counted).  CFF2 outlines, and everything built from them, are
	// drawn there, `glyf` outlines are moved by `gvar` (G1 to G6 below), and glyph_hor_advance follows `HVAR`.  Refused (nullopt,
	// *err says why): a file without a readable `fvar`, a face whose outlines are `glyf` without a readable `gvar` (version 1.0,
	// axisCount equal to fvar's, the header, the shared tuples and the offset array inside the table), a coordinate count other
	// than the axes', an `HVAR` whose store is not of format 1 or holds 32-bit deltas (LONG_WORDS).  An `HVAR` that cannot be
	// read at all (major version not 1, a header, store header or region list outside the table) counts as absent, as the crate
	// drops it; without `HVAR` the `hmtx` advance stands, unless the face is `glyf` + `gvar` and was placed with gvar_advances
	// on: then its advances follow gvar's phantom points (G7 below).
	//
	// A `glyf` face at a position: outline_glyph, outline_glyph_packed and command_table() deliver the outline there.  The rules
	// are the OpenType specification's; where it leaves the f32 order open, the order below is the definition.
	// G1, glyph data.  Glyph id g owns the `gvar` bytes [offset[g], offset[g+1]) behind glyphVariationDataArrayOffset, in the
	//   short (times 2) or the long offset form.  A glyph id at or past glyphCount, or with an empty range, has no deltas; a
	//   range that descends or leaves the table is malformed.  tupleVariationCount: bit 0x8000 = shared point numbers (they
	//   stand first in the serialized data, and are read whenever the bit is set), the low 12 bits the count (0: no deltas);
	//   dataOffset follows.  Each tuple header holds variationDataSize and tupleIndex — 0x8000 an embedded peak, 0x4000
	//   intermediate start and end, 0x2000 private point numbers, the low 12 bits the shared tuple index — and the tuples' data
	//   lie one behind the other from dataOffset (behind the shared point numbers) on, variationDataSize bytes each, whether
	//   the tuple is applied or skipped.
	// G2, packed point numbers.  A count byte of 0: all points.  Bit 7 set: the two-byte count form (a count of 0 in that form
	//   lists no point).  Runs of 1 to 128 values (control byte: bit 7 = 16-bit values, low 7 bits + 1 the length; a run is read
	//   as far as the count goes), increments summed in u16.  Numbers that are not strictly ascending make the glyph's data
	//   malformed; a number at or past the point count names no point (its deltas are read and dropped).  A tuple with neither
	//   private nor shared numbers is over all points.
	// G3, packed deltas.  One stream of 2 * count values, the x deltas first: a control byte — 0x80 a zero run, 0x40 a word
	//   run, else a byte run, the low 6 bits + 1 the run length — and the run's values.
	// G4, scalar of a tuple.  The f32 product over the axes, in axis order, of axis_factor(coord, start, peak, end) (cff.hpp);
	//   without an intermediate region start = min(peak, 0) and end = max(peak, 0).  A tuple whose scalar is 0 is skipped (its
	//   point numbers and deltas are not looked at).  A shared tuple index at or past sharedTupleCount makes the data malformed.
	// G5, simple glyph of n points (+ 4 phantom points, numbered n .. n + 3).  An accumulator (ax, ay) per point starts at 0;
	//   tuples are applied in order; a touched point gets a += f32(delta) * scalar, one product and one sum.  A tuple over all
	//   points touches every point.  A tuple over a subset leaves the other points of a contour to inference, x and y each on
	//   its own, from the nearest touched points before and behind it in the contour (cyclic) and the ORIGINAL INTEGER
	//   coordinates: with pa / da of the touched point before, pb / db of the one behind (da, db already scaled) and p the
	//   target — pa == pb: da if da == db, else 0; p <= min(pa, pb): the delta of the smaller of the two coordinates;
	//   p >= max(pa, pb): that of the larger; otherwise d = f32(p - pa) / f32(pb - pa) and (1 - d) * da + d * db in f32 — and the
	//   result is added as a touched point's would be.  A contour without a touched point gets nothing from that tuple; phantom
	//   points are never inferred.  The point is then f32(i16 coordinate) + a; everything behind that is the static walk's
	//   (transform, implied midpoints, closing curve).  Contours are those of the static walk's own end-point iterator.
	// G6, composite glyph.  One point per component record the static walk reads, in record order, + 4 phantom points; touched
	//   points only, no inference.  Component k's e and f, as the static walk has them, get += a in f32 before the transform is
	//   combined with the parent's.  Children vary by their own data.
	// G7, advance from the phantom points.  Followed by a face placed with gvar_advances on that has no readable `HVAR` (`HVAR`
	//   wins whenever it is there).  Point count n of glyph id g's OWN entry: a simple entry (numberOfContours > 0) has its last
	//   end point + 1 (only the end points are read: whether the flags and coordinates behind them are sound is the outline's
	//   matter); an entry of numberOfContours 0 has 0; a composite has one point per component record the static walk reads;
	//   a glyph id WITHOUT an entry (Face::glyph_data has none: a `loca` range of length 0, `space` for instance, or one that
	//   descends or leaves `glyf`) has n = 0 and still its four phantom points.  An entry whose count cannot be read — shorter
	//   than 2 bytes, a simple or composite one shorter than 10, end points that leave the entry, a last end point of 0xFFFF — is
	//   malformed.  Two f32 accumulators l (point n, x) and r (point n + 1, x) start at 0.  The glyph's tuples are taken in order
	//   by G1 to G4, a tuple of scalar 0 skipped unread.  An applied tuple over all points contributes its x deltas number n and
	//   n + 1; one with point numbers, private or shared, the x delta at the position in its list where n or n + 1 is named, and
	//   nothing for a number not named; each contribution is += f32(delta) * scalar, one product and one sum, as in G5.  Phantom
	//   points are never inferred.  d = r - l, one f32 subtraction, stands where `HVAR`'s delta stands in glyph_hor_advance:
	//   (f32)hmtx advance + (d + 0.5), truncated, none outside 0 .. 65535.  A glyph id at or past glyphCount, with an empty
	//   range of `gvar` or with tuple count 0 has d = 0.  Malformed data, by G1 to G5's meaning at that position — every applied
	//   tuple's point numbers and all 2 * count of its deltas are walked, not only those up to n + 1 — or a malformed entry
	//   gives no delta: the `hmtx` advance stands.  In this reader G1 to G4 are one function (GvarTable::applied_tuples), which
	//   the outline's accumulation and this rule's sums both call; the device still states them once in its accumulate and once
	//   in its phantom_sums (profiles/gvar_tuple_walk_ab.txt says why).  NOT BUILT: USE_MY_METRICS is not consulted
	//   (a composite's phantom points take the composite's own data, as fontTools does); the outline is not shifted by the left
	//   phantom point, as it is not under `HVAR`; the vertical phantom points (n + 2, n + 3) are not read.
	// Malformed data of a glyph id — a header, point numbers or deltas that leave the glyph's range, a tuple that ends before
	// its deltas do — delivers nothing from where the data is needed: outline_glyph returns false there, leaves delivered
	// before it stay.  PARITY UNPINNED like the rest of the variation code; checked against fontTools and a strict restatement
	// (tests/test_gvar_instances_host.py).
	static std::optional<Face> parse_at(const uint8_t *data, size_t len, const std::vector<int16_t> &coords, std::string *err = nullptr,
	                                    bool gvar_advances = false);
	// made by parse_at (even at all-zero coordinates)
	bool at_position() const { return at_position_; }
	// THE predicate of G7: placed with gvar_advances on, by gvar, and without a readable `HVAR`
	bool advances_by_gvar() const { return gvar_advances_ && gvar_ != nullptr && hvar_.empty(); }
	// G7 for one glyph id of a face placed by gvar, whether or not its advances follow it (test / inspection, and what the
	// device's phantom pass is held to): the state — kGvarAdvanceNone (no variation data: d = 0), kGvarAdvanceDelta,
	// kGvarAdvanceMalformed (d = 0: not to be used) — and d.  A streaming walk: no per-point storage, nothing inferred.
	enum : uint8_t { kGvarAdvanceNone = 0, kGvarAdvanceDelta = 1, kGvarAdvanceMalformed = 2 };
	uint8_t gvar_advance_delta(uint16_t glyph_id, float &d) const;
	const std::vector<int16_t> &coords() const { return coords_; }
	// every glyph id's glyph_hor_advance().value_or(0), for ids 0 .. n - 1 (test / inspection: ids at and past numGlyphs give 0)
	std::vector<uint16_t> hor_advances(uint32_t n) const;
	// parse_at with an `HVAR`: the factor of every region of its store at the face's position, evaluated once
	const std::vector<float> &hvar_region_scalars() const { return hvar_scalars_; }
	// ... and the offset `HVAR` has for the glyph's advance there (nullopt: none — no map entry, an index outside the store, a
	// row that leaves the table): the sum over the row's columns of delta * factor, one f32 product and one f32 sum each
	std::optional<float> hvar_advance_delta(uint16_t glyph_id) const;

	uint16_t units_per_em() const { return units_per_em_; }
	uint16_t number_of_glyphs() const { return num_glyphs_; }
	std::optional<uint16_t> glyph_index(uint32_t code_point) const;
	// (a face made by parse_at: (f32)advance + delta + 0.5, truncated; outside 0 .. 65535: none)
	std::optional<uint16_t> glyph_hor_advance(uint16_t glyph_id) const;
	// Emits the glyph's outline; returns false when ttf-parser would return None
	// (callbacks already delivered stay delivered, as in the crate).
	bool outline_glyph(uint16_t glyph_id, OutlineBuilder &builder) const;
	// The same callbacks appended to `kinds` / `coords` in the compact upload form of vgsdf_outlines_packed (kind byte
	// 0..4 = move / line / quad / curve / close + the coordinates the kind carries); glyf outlines are walked with the sink
	// inlined (no virtual call per point).
	bool outline_glyph_packed(uint16_t glyph_id, std::vector<uint8_t> &kinds, std::vector<float> &coords) const;
	// glyf fonts only (has_glyf_form()): the same walk up to the simple glyphs, which are not decoded but appended as
	// parts — their bytes to `bytes` (4-aligned), their command slots counted from `slots` on.  false: ttf-parser returns
	// None at this point (parts appended so far stay, as the callbacks delivered so far would).  *overflow is set (and the
	// walk stops) when the batch would pass what its 32-bit offsets address (2^26 bytes / slots, 2^22 parts per recorder): a composite
	// copies its simple glyphs once per leaf, so a small font can fan out to gigabytes — the caller then drops the glyf form.
	bool glyph_parts(uint16_t glyph_id, std::vector<GlyfPart> &parts, std::vector<uint8_t> &bytes, uint32_t &slots, bool *overflow = nullptr) const;
	// The resident form of the face: built once, on first use (thread-safe); the same walk and the same checks as
	// glyph_parts, glyph id by glyph id, so a failing component leaves a glyph with the leaves recorded so far.
	const ResidentTable &resident_table() const;
	// What a renderer keys the face's glyf-kind device font by, whichever way the font is made (resident_table().serial is this
	// number when the table is ok); handed out on first use, without building the table.
	uint64_t resident_serial() const;
	// The command form of the face: built once, on first use (thread-safe), by the very call Renderer::record makes for a
	// glyph (outline_glyph_packed, return value ignored) for every glyph id.  The callbacks are counted first and the count stops at the
	// bounds, so a face past them is refused without its table ever being allocated.
	const CommandTable &command_table() const;
	// What a renderer keys the face's command store by, whichever way the store is made (command_table().serial is this number);
	// handed out on first use, without building a table.
	uint64_t command_serial() const;
	// The charstring form of a `CFF ` version 1 face: built once, on first use (thread-safe), from the tables CffTable::parse has
	// located — no charstring is interpreted.
	const CharstringTable &charstring_table() const;
	// The same of a `CFF2` face, with its blend sets (not ok for every other face, and for one whose local subroutines are more
	// than the description's 65535).
	const CharstringTable &charstring2_table() const;
	// The face's loca and glyf for the device's table builder (the resident form without the host walking a glyph).
	FontTables font_tables() const;
	// A face placed by gvar: its loca, glyf and gvar and its coordinates for the device's builder of its command store — the host
	// half of vgsdf_font_create_gvar, as font_tables() is of vgsdf_font_create_tables.
	GvarTables gvar_tables() const;
	// The face's tables for the device's family-table kernels: built once, on first use (thread-safe).
	const FamilyTables &family_tables() const;
	// ttf-parser's `tables().cmap.is_some()`; the reference refuses fonts without one (metadata.rs:104-107)
	bool has_cmap() const { return has_cmap_; }
	// glyph outlines this reader can emit: `glyf` + `loca`, or `CFF ` charstrings (ttf-parser's order: glyf first).
	// A font whose outlines live in a table this reader cannot walk (`CFF2`, or a `CFF ` table it fails to parse)
	// is refused at load time instead of yielding empty glyphs.
	bool has_glyf_outlines() const { return !glyf_.empty() && !loca_.empty(); }
	// made by parse_at from `glyf` + `gvar`: the entries of `glyf` are NOT the face's outlines as they stand
	bool placed_by_gvar() const { return gvar_ != nullptr; }
	// THE predicate of every form that reads `glyf` entries as outlines (glyph_parts, resident_table, font_tables, the glyf
	// stores and the glyf submission form, a font id's say in mixing): a face placed by gvar has none of them and is a command
	// face everywhere
	bool has_glyf_form() const { return has_glyf_outlines() && !placed_by_gvar(); }
	bool has_cff_outlines() const { return cff_ != nullptr; }
	bool has_unsupported_outlines() const { return !has_glyf_outlines() && !cff_ && cff_unreadable_; }
	// Face::names() (src/font/metadata.rs:92-97): every record of the `name` table in table order as
	// (name_id, Name::to_string().unwrap_or_default()): UTF-16BE records of the Unicode platform and of
	// the Windows platform (encodings 0 and 1) decoded to UTF-8, every other record an empty string.
	std::vector<std::pair<uint16_t, std::string>> names() const;
	// Sorted unique code points that a unicode cmap subtable maps to a glyph.
	std::vector<uint32_t> unicode_codepoints() const;

private:
	struct CmapSubtable {
		uint16_t platform = 0, encoding = 0, format = 0xFFFF;
		Bytes data; // from the subtable start to the end of the cmap table
		uint32_t offset = 0; // of the subtable in the cmap table
		bool is_unicode() const;
		std::optional<uint16_t> glyph_index(uint32_t cp) const;
		template <class F> void for_each_codepoint(F &&f) const;
	};

	std::optional<Bytes> glyph_data(uint16_t glyph_id) const;
	static std::optional<Face> parse_impl(const uint8_t *data, size_t len, const std::vector<int16_t> *coords, std::string *err);
	// G7's point count of the glyph id's own entry; false: the entry is malformed
	bool own_point_count(uint16_t glyph_id, uint32_t &n) const;

	Bytes hmtx_, loca_, glyf_, name_, cmap_table_;
	bool at_position_ = false, gvar_advances_ = false;
	std::vector<int16_t> coords_;
	Bytes hvar_;                      // parse_at: the table when its store can be read, else empty
	uint32_t hvar_store_ = 0, hvar_map_ = 0;
	std::vector<float> hvar_scalars_; // one per region of the store
	std::vector<CmapSubtable> cmap_;
	uint16_t units_per_em_ = 0, num_glyphs_ = 0, num_hmetrics_ = 0;
	bool loca_long_ = false, has_cmap_ = false, cff_unreadable_ = false;
	std::shared_ptr<const CffTable> cff_;
	std::shared_ptr<const GvarTable> gvar_; // parse_at of a `glyf` face
	size_t loca_entries_ = 0;
	struct ResidentCell {
		std::once_flag once, serial_once;
		uint64_t serial = 0;
		ResidentTable table;
	};
	std::shared_ptr<ResidentCell> resident_ = std::make_shared<ResidentCell>(); // (shared by copies of the Face: same bytes)
	struct CommandCell {
		std::once_flag once, serial_once, charstrings_once, charstrings2_once;
		uint64_t serial = 0;
		CommandTable table;
		CharstringTable charstrings, charstrings2;
	};
	std::shared_ptr<CommandCell> commands_ = std::make_shared<CommandCell>();
	struct FamilyCell {
		std::once_flag once;
		FamilyTables tables;
	};
	std::shared_ptr<FamilyCell> family_ = std::make_shared<FamilyCell>();

	template <class B, bool PARTS> friend struct GlyfWalker;
	template <class B> friend struct GvarWalker;
};

} // namespace vg
