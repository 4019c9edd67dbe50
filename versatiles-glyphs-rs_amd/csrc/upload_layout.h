// upload_layout.h — byte offsets of the single-block upload forms.  include/vgsdf.h states the two layouts for callers
// (vgsdf_outlines_packed, vgsdf_outlines_glyf); this header is their one computation (and that of the
// block the library itself gathers for vgsdf_outlines_resident), used by the host façade that
// builds such a block (csrc/host/renderer.hpp, MergedOutlines) and by the front-end that recognises one, sizes its
// device copy and derives the device views from it (outline_front_end.cpp).  Plain C++: no HIP here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vgsdf.h"

namespace vgsdf {

// scale f64[n] | shift_x f64[n] | cmd_off u32[n + 1]: the head of both forms, and all of the per-glyph arrays of the
// plain command form
struct GlyphArraysLayout {
	size_t scale = 0, shift_x, cmd_off, end;
	explicit GlyphArraysLayout(size_t n) : shift_x(8 * n), cmd_off(16 * n), end(16 * n + 4 * (n + 1)) {}
};

// ... | dat_off u32[n + 1] | pad to 8 | coords f32[n_floats] | kinds u8[n_cmds] [| pad to 4 | pbf_pre u32[n] | pbf_fix u8[n]]
struct PackedBlockLayout : GlyphArraysLayout {
	size_t dat_off, arrays_end; // arrays_end: behind the per-glyph arrays
	size_t coords, kinds, pbf_pre, pbf_fix, bytes;
	PackedBlockLayout(size_t n, size_t n_cmds, size_t n_floats, bool with_pbf) : GlyphArraysLayout(n)
	{
		dat_off = end;
		arrays_end = dat_off + 4 * (n + 1);
		coords = (arrays_end + 7) / 8 * 8;
		kinds = coords + 4 * n_floats;
		pbf_pre = (kinds + n_cmds + 3) / 4 * 4;
		pbf_fix = pbf_pre + 4 * n;
		bytes = with_pbf ? pbf_fix + n : kinds + n_cmds;
	}
};

// ... | pad to 8 | parts vgsdf_glyf_part[n_parts] | bytes u8[n_bytes] (a multiple of 4) [| pbf_pre u32[n] | pbf_fix u8[n]]
struct GlyfBlockLayout : GlyphArraysLayout {
	size_t parts, glyf_bytes, pbf_pre, pbf_fix, bytes;
	GlyfBlockLayout(size_t n, size_t n_parts, size_t n_bytes, bool with_pbf) : GlyphArraysLayout(n)
	{
		parts = (end + 7) / 8 * 8;
		glyf_bytes = parts + sizeof(vgsdf_glyf_part) * n_parts;
		pbf_pre = glyf_bytes + n_bytes;
		pbf_fix = pbf_pre + 4 * n;
		bytes = with_pbf ? pbf_fix + n : pbf_pre;
	}
};

// The form that names its glyphs (vgsdf_outlines_resident):
// ... | part_off u32[n + 1] | glyph_id u16[n] | font_of u16[n] [| pbf_pre u32[n] | pbf_fix u8[n]] = 33 n + 8 bytes with the
// PBF arrays, then (16-aligned) 32 bytes of device addresses per font the submission names, and the whole padded to 16.
// The device keeps a copy of the block as it stands and, behind it, the parts the upload kernel expands the leaves into.
struct ResidentFontRef { // a resident font's three arrays (device addresses)
	uint64_t leaf_off, leaves, bytes, reserved;
};
struct ResidentBlockLayout : GlyphArraysLayout {
	size_t part_off, glyph_id, font_of, pbf_pre, pbf_fix, arrays_end, fonts, bytes; // bytes: the block; the parts follow on the device
	ResidentBlockLayout(size_t n, size_t n_fonts, bool with_pbf) : GlyphArraysLayout(n)
	{
		part_off = end;
		glyph_id = part_off + 4 * (n + 1);
		font_of = glyph_id + 2 * n;
		pbf_pre = font_of + 2 * n;
		pbf_fix = pbf_pre + 4 * n;
		arrays_end = with_pbf ? pbf_fix + n : pbf_pre;
		fonts = (arrays_end + 15) / 16 * 16;
		bytes = fonts + sizeof(ResidentFontRef) * n_fonts; // (a multiple of 16)
	}
};

// The same form against command fonts (vgsdf_font_create_commands): a glyph's commands lie expanded in its font's store, so
// the block needs no second running sum:
// ... | glyph_id u16[n] | font_of u16[n] [| pbf_pre u32[n] | pbf_fix u8[n]] = 29 n + 4 bytes with the PBF arrays, then
// (16-aligned) 32 bytes of device addresses per font, the whole a multiple of 16.  The upload kernel copies the block and
// gathers every named glyph's records and context bytes behind cmd_off[g] of the batch's command arrays.
struct CommandFontRef { // a command font's three arrays (device addresses)
	uint64_t cmd_off, cmds, open, reserved; // u32[n_glyph_ids + 1] | 28-byte records | the context pass's byte per record
};
static_assert(sizeof(CommandFontRef) == sizeof(ResidentFontRef), "one size of font reference in every block that names fonts");
// The kind of a font reference, in its `reserved` word.  0: the block's own kind — every block of the forms above, whose lists
// hold ONE kind.  The mixed forms (vgsdf_outlines_submit_resident_mixed, mixed families) keep fonts of both kinds in one list
// of ResidentBlockLayout and say which a reference is; a command glyph has no parts there (part_off stands still over it) and
// cmd_off runs over the glyphs of both kinds.
constexpr uint64_t kFontRefOfBlock = 0, kFontRefGlyf = 1, kFontRefCommands = 2;
// a reference of such a list, read as either kind (the three addresses share their places)
struct MixedFontRef {
	uint64_t a, b, c, kind;
#if defined(__HIPCC__)
	__host__ __device__
#endif
	    operator ResidentFontRef() const
	{
		return ResidentFontRef{a, b, c, kind};
	}
#if defined(__HIPCC__)
	__host__ __device__
#endif
	    operator CommandFontRef() const
	{
		return CommandFontRef{a, b, c, kind};
	}
};
static_assert(sizeof(MixedFontRef) == sizeof(ResidentFontRef), "one size of font reference in every block that names fonts");
struct CommandBlockLayout : GlyphArraysLayout {
	size_t glyph_id, font_of, pbf_pre, pbf_fix, arrays_end, fonts, bytes;
	CommandBlockLayout(size_t n, size_t n_fonts, bool with_pbf) : GlyphArraysLayout(n)
	{
		glyph_id = end;
		font_of = glyph_id + 2 * n;
		pbf_pre = font_of + 2 * n;
		pbf_fix = pbf_pre + 4 * n;
		arrays_end = with_pbf ? pbf_fix + n : pbf_pre;
		fonts = (arrays_end + 15) / 16 * 16;
		bytes = fonts + sizeof(CommandFontRef) * n_fonts; // (a multiple of 16)
	}
};

// The stores those references point into: one device allocation per font, laid out the same by every constructor of a kind
// (resident_*.cpp), so the same face takes the same vgsdf_font_device_bytes whichever way it was built.  A glyf font:
//   leaves vgsdf_glyf_part[n_leaves] | bytes u8[n_bytes] (a multiple of 4) | pad to 16 | leaf_off u32[n_glyph_ids + 1]
struct GlyfStoreLayout {
	size_t leaves = 0, bytes, leaf_off, total;
	constexpr GlyfStoreLayout(size_t n_glyph_ids, size_t n_leaves, size_t n_bytes)
	    : bytes(sizeof(vgsdf_glyf_part) * n_leaves), leaf_off((bytes + n_bytes + 15) / 16 * 16), total(leaf_off + 4 * (n_glyph_ids + 1))
	{
	}
};
// A command font: records (28 bytes each) [n_cmds] | cmd_off u32[n_glyph_ids + 1] | open u8[n_cmds] (the context pass's byte per
// record) = 29 n_cmds + 4 (n_glyph_ids + 1) bytes; `total` is also what the 32-bit offsets of a store are checked against
struct CommandStoreLayout {
	size_t cmds = 0, cmd_off, open, total;
	constexpr CommandStoreLayout(size_t n_glyph_ids, size_t n_cmds)
	    : cmd_off(28 * n_cmds), open(cmd_off + 4 * (n_glyph_ids + 1)), total(open + n_cmds)
	{
	}
};
static_assert(sizeof(vgsdf_glyf_part) == 48, "a leaf of a glyf store");
static_assert(GlyfStoreLayout(5, 3, 16).bytes == 144 && GlyfStoreLayout(5, 3, 16).leaf_off == 160 && GlyfStoreLayout(5, 3, 16).total == 184 &&
                  GlyfStoreLayout(5, 3, 20).leaf_off == 176 && GlyfStoreLayout(5, 3, 24).leaf_off == 176 && GlyfStoreLayout(5, 3, 28).leaf_off == 176 &&
                  GlyfStoreLayout(5, 3, 28).total == 200 && GlyfStoreLayout(7, 0, 0).leaf_off == 0 && GlyfStoreLayout(7, 0, 0).total == 32 &&
                  GlyfStoreLayout(0, 0, 0).total == 4 && GlyfStoreLayout(0, 1, 4).leaf_off == 64 && GlyfStoreLayout(0, 1, 4).total == 68,
              "leaves | bytes | pad to 16 | leaf_off, at n_bytes = 0, 4, 8, 12 (mod 16), without leaves and without glyph ids");
static_assert(CommandStoreLayout(3, 10).cmd_off == 280 && CommandStoreLayout(3, 10).open == 296 && CommandStoreLayout(3, 10).total == 29 * 10 + 4 * 4 &&
                  CommandStoreLayout(65, 0).cmd_off == 0 && CommandStoreLayout(65, 0).open == 264 && CommandStoreLayout(65, 0).total == 264 &&
                  CommandStoreLayout(0, 0).total == 4 && CommandStoreLayout(0x10000, 0x8000000).total == 29ull * 0x8000000 + 4ull * 0x10001,
              "records | cmd_off | open: 29 bytes per command and 4 per glyph id + 4, without commands and without glyph ids");

// The form that names code-point RANGES of resident families (vgsdf_outlines_ranges).  A family's table lives on the device
// (resident_families.cpp, vgsdf_family_create), one allocation of arrays over its n entries:
//   scale f64[n] | shift_x f64[n] | cmd_pre u32[n + 1] | leaf_pre u32[n + 1] | advance u32[n] | code_point u16[n] |
//   font_of u16[n] | glyph_id u16[n] | pbf_fix u8[n]
// cmd_pre / leaf_pre: prefix sums over the entries of their glyphs' command slots / leaves, mod 2^32 (a submission holds fewer
// than 2^31 of either, so differences are exact).  Used by the host and, with the entry count of the block's family record,
// by the upload kernels (constexpr: callable on the device).
struct FamilyTableLayout {
	size_t scale = 0, shift_x, cmd_pre, leaf_pre, advance, code_point, font_of, glyph_id, pbf_fix, bytes;
	constexpr explicit FamilyTableLayout(size_t n)
	    : shift_x(8 * n), cmd_pre(16 * n), leaf_pre(16 * n + 4 * (n + 1)), advance(16 * n + 8 * (n + 1)), code_point(20 * n + 8 * (n + 1)),
	      font_of(22 * n + 8 * (n + 1)), glyph_id(24 * n + 8 * (n + 1)), pbf_fix(26 * n + 8 * (n + 1)), bytes(27 * n + 8 * (n + 1))
	{
	}
};
// The block of such a submission: 32 bytes per task that maps a glyph, per family and per font, nothing per glyph —
//   RangeTask[n_live] | FamilyRef[n_families] | font references[n_fonts] (ResidentFontRef or CommandFontRef; a submission of mixed
//   families: MixedFontRef, each saying its kind, and the device's copy is ResidentBlockLayout's)
// The upload kernel of the form WRITES the per-glyph arrays of ResidentBlockLayout / CommandBlockLayout into the device's copy
// (where every later kernel reads them) and copies the font references to that layout's `fonts`.
struct RangeTask {
	uint32_t glyph_base;  // the task's first glyph in the submission (ascending over the block's tasks: they are bisected)
	uint32_t n_glyphs;    // > 0: tasks that map nothing are not in the block
	uint32_t entry_first; // its first entry in the family's table
	uint32_t family;      // index into the block's family records
	uint32_t cmd_rel;     // the task's first command slot in the batch - cmd_pre[entry_first] (mod 2^32)
	uint32_t part_rel;    // glyf fonts: the task's first part - leaf_pre[entry_first] (mod 2^32)
	uint32_t pbf_pre;     // bytes reserved in front of the task's first glyph entry
	uint32_t reserved;
};
struct FamilyRef {
	uint64_t table;     // device address of the family's table
	uint32_t n_entries; // (what FamilyTableLayout is made from)
	uint32_t font_base; // where the family's fonts begin in the block's font list
	uint32_t n_fonts;
	uint32_t cp_base; // the family's plane << 16: an entry's id is cp_base + its code_point
	uint32_t reserved[2];
};
static_assert(sizeof(RangeTask) == 32 && sizeof(FamilyRef) == 32, "one record size throughout the block");
struct RangesBlockLayout {
	size_t tasks = 0, families, fonts, bytes;
	RangesBlockLayout(size_t n_live, size_t n_families, size_t n_fonts)
	    : families(32 * n_live), fonts(32 * (n_live + n_families)), bytes(32 * (n_live + n_families + n_fonts))
	{
	}
};
// what the upload kernel leaves per glyph for pbf_entries (device only): the entry's id (its code point) and advance, and
// 1 + the index of the block's task whose first glyph this is (0: not a first glyph)
struct EntryName {
	uint32_t id, advance, task_first, reserved;
};

} // namespace vgsdf
