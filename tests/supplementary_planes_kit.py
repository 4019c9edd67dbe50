"""What the tests of the supplementary planes share (no test in here): hand-written `cmap` tables whose spans reach past
U+FFFF (built with tests/cmap_edge_tables.py's builders), and strict Python restatements of

  the entries of plane p of a family: for every code point c of [(p << 16), (p << 16) + 0xFFFF] outside the surrogates the first
  face that MAPS it (a unicode subtable enumerates it and that subtable's lookup has a value), the first value any subtable of
  that face has, advance, scale and shift_x in f64; the table keeps c's low half and pbf_fix counts the varint of the full c;

  the census of the tables (include/vgsdf.h, vgsdf_family_tables_census): bit b of 4352 set exactly when some subtable LISTS a
  code point of [256 b, 256 b + 255] that is no surrogate and at most 0x10FFFF — format 0: c < 256 when the table has its 262
  bytes; format 4: the segments less a closing 0xFFFF - 0xFFFF; formats 6 and 10: [first, first + count - 1]; 12 and 13: the groups.

The lookups are cmap_edge_tables._Sub.look, which follows the host reader for any code point.  No tolerance appears anywhere."""
import numpy as np

import cmap_edge_tables as E
from cmap_edge_tables import PAST, SENTINEL, SMALL, face, fmt4, fmt10, fmt12, plain_face, u16, u32

PLANES = (0, 1, 16)
CENSUS_BLOCKS = 0x110000 // 256
CENSUS_WORDS = CENSUS_BLOCKS // 32
SURROGATE_BLOCKS = range(0xD8, 0xE0)


# ---- the restatements ----

def enumerated(sub):
    """Face::CmapSubtable::for_each_codepoint as inclusive ranges, NOT clipped to the BMP (format 6 ends at 0xFFFF, format 10
    where first + k would wrap)"""
    d, fmt, out = sub.d, sub.fmt, []
    if fmt == 0 and sub.has(6, 256):
        out = [(c, c) for c in range(256) if d[6 + c]]
    elif fmt == 4 and sub._f4() is not None:
        segs, ends, starts, _, _ = sub._f4()
        for s in range(segs):
            a, b = u16(d, starts + s * 2), u16(d, ends + s * 2)
            if a == 0xFFFF and b == 0xFFFF:
                break
            out.append((a, b))
    elif fmt == 6 and sub.has(0, 10):
        out = [(u16(d, 6), min(u16(d, 6) + u16(d, 8) - 1, 0xFFFF))]
    elif fmt == 10 and sub.has(0, 20):
        out = [(u32(d, 12), min(u32(d, 12) + u32(d, 16) - 1, 0xFFFFFFFF))]
    elif fmt in (12, 13) and sub.has(0, 16) and sub.has(16, u32(d, 12) * 12):
        out = [(u32(d, 16 + k * 12), u32(d, 20 + k * 12)) for k in range(u32(d, 12))]
    return [(a, b) for a, b in out if a <= b]


def face_map_plane(t, plane):
    """{code point: glyph id} of one face description over the code points of `plane`"""
    lo, hi = plane << 16, (plane << 16) + 0xFFFF
    subs = [E._Sub(t["cmap"], int(o), int(f)) for o, f in zip(t["subtable_off"], t["subtable_format"])]
    out = {}
    for s in subs:
        for a, b in enumerated(s):
            for c in range(max(a, lo), min(b, hi) + 1):
                if c in out or 0xD800 <= c <= 0xDFFF or s.look(c) is None:
                    continue
                out[c] = next(g for g in (x.look(c) for x in subs) if g is not None)
    return out


def restate_plane(faces, plane):
    """the entries of plane `plane` of the family of `faces` (descriptions, provider order), as cmap_edge_tables.restate gives
    plane 0's: code_point the LOW halves, pbf_fix from the full code point; full: the code points themselves"""
    owner = {}
    for k, t in enumerate(faces):
        for c, g in face_map_plane(t, plane).items():
            owner.setdefault(c, (k, g))
    cps = sorted(owner)
    font_of, gid, adv, scale, shift, fix = [], [], [], [], [], []
    for c in cps:
        k, g = owner[c]
        t = faces[k]
        s = 24.0 / float(t["units_per_em"])
        af = float(E.hor_advance(t, g)) * s * 0.95
        a = E.round_half_away(af)
        font_of.append(k), gid.append(g), adv.append(a), scale.append(s), shift.append((float(a) - af) / 2.0)
        fix.append((1 + E.varint_len(c)) | ((1 + E.varint_len(a)) << 4))
    return {"code_point": np.array([c & 0xFFFF for c in cps], np.uint16), "font_of": np.array(font_of, np.uint16),
            "glyph_id": np.array(gid, np.uint16), "advance": np.array(adv, np.uint32), "scale": np.array(scale, np.float64),
            "shift_x": np.array(shift, np.float64), "pbf_fix": np.array(fix, np.uint8), "full": np.array(cps, np.uint32)}


def census_listed(sub):
    """the spans a subtable lists by the census's definition"""
    d, fmt = sub.d, sub.fmt
    if fmt == 0:
        return [(0, 255)] if sub.has(6, 256) else []
    if fmt == 4:
        t = sub._f4()
        if t is None:
            return []
        segs, ends, starts, _, _ = t
        spans = [(u16(d, starts + s * 2), u16(d, ends + s * 2)) for s in range(segs)]
        return [s for s in spans if s != (0xFFFF, 0xFFFF)]
    if fmt == 6:
        return [(u16(d, 6), u16(d, 6) + u16(d, 8) - 1)] if sub.has(0, 10) else []
    if fmt == 10:
        return [(u32(d, 12), u32(d, 12) + u32(d, 16) - 1)] if sub.has(0, 20) else []
    if fmt in (12, 13) and sub.has(0, 16) and sub.has(16, u32(d, 12) * 12):
        return [(u32(d, 16 + k * 12), u32(d, 20 + k * 12)) for k in range(u32(d, 12))]
    return []


def census_blocks(faces):
    """the set of blocks b whose bit the census sets for `faces` (descriptions)"""
    blocks = set()
    for t in faces:
        for o, f in zip(t["subtable_off"], t["subtable_format"]):
            for a, b in census_listed(E._Sub(t["cmap"], int(o), int(f))):
                b = min(b, 0x10FFFF)
                # what the span lists on either side of the surrogates
                for lo, hi in ((a, min(b, 0xD7FF)), (max(a, 0xE000), b)):
                    if lo <= hi:
                        blocks.update(range(lo >> 8, (hi >> 8) + 1))
    return blocks


def census_bits(blocks):
    bits = np.zeros(CENSUS_WORDS, np.uint32)
    for b in blocks:
        bits[b >> 5] |= np.uint32(1 << (b & 31))
    return bits


def blocks_of_bits(bits):
    return {32 * w + k for w in range(len(bits)) for k in range(32) if (int(bits[w]) >> k) & 1}


# ---- the expected PBF of a supplementary block ----

class OracleFonts:
    """the files of a font id as the oracle reads them, in provider order (vgo_render_block's provider table is BMP only)"""

    def __init__(self, O, paths_or_bytes):
        self.O = O
        self.fonts = [O.Font(p) for p in paths_or_bytes]
        self.maps = [set(int(c) for c in f.codepoints()) for f in self.fonts]

    def blocks(self):
        """{start: code points} of the populated supplementary blocks, first provider wins"""
        out = {}
        for m in self.maps:
            for c in m:
                if 0xFFFF < c <= 0x10FFFF:
                    out.setdefault(c & ~0xFF, set()).add(c)
        return {s: sorted(v) for s, v in sorted(out.items())}

    def block_pbf(self, name, start, mode):
        """Font.render_glyph per code point of [start, start + 255] by its first provider, then oracle.pbf_encode"""
        glyphs = []
        for c in range(start, start + 256):
            k = next((k for k, m in enumerate(self.maps) if c in m), None)
            if k is None:
                continue
            g = self.fonts[k].render_glyph(c, mode)
            if g is not None:
                glyphs.append(g)
        return self.O.pbf_encode(name, start, glyphs)


# the supplementary blocks of the 20-file Noto Sans id: Noto Sans Regular U+10700, U+1DF00 (88 code points), Sinhala U+11100
# (20), Tamil U+11300 (4), Ethiopic U+1E700 (28)
NOTO_BLOCKS = (0x10700, 0x11100, 0x11300, 0x1DF00, 0x1E700)
NOTO_CODE_POINTS = 140


# ---- the tables ----

LANE_EDGES = [0x10000, 0x1003F, 0x10040, 0x100FF, 0x10100, 0x1FFFF]     # first lane, wave edge, workgroup edge, last lane of the grid


def edge_cases():
    """name -> faces (provider order): regular tables whose spans reach past U+FFFF.  Glyph ids come from the synthetic fonts of
    family_ranges_kit (SMALL); where a table by its nature names ids past them the build of that plane is refused by both
    constructors alike"""
    c = {}
    c["f12_inside_plane_1"] = [face([(3, 10, fmt12([(0x10400, 0x10409, 4)]))])]
    c["f12_across_the_plane_edge"] = [face([(3, 10, fmt12([(0xFFF8, 0x10007, 2)]))])]
    # ... and from U+FFF0 to U+1000F: 32 consecutive glyph ids, more than the synthetic fonts have, so plane 1 of it is refused
    c["f12_fff0_to_1000f"] = [face([(3, 10, fmt12([(0xFFF0, 0x1000F, 0)]))])]
    c["f12_across_the_surrogates"] = [face([(3, 10, fmt12([(0xD7F0, 0xE00F, 0)]))])]
    c["f13_across_the_surrogates"] = [face([(0, 4, fmt12([(0xD7F0, 0xE00F, 5)], fmt=13))])]
    c["f12_ends_at_10ffff_and_at_ffffffff"] = [face([(3, 10, fmt12([(0x10FFF0, 0x10FFFF, 3), (0x110000, 0xFFFFFFFF, 1)]))])]
    c["f13_ends_at_ffffffff"] = [face([(0, 4, fmt12([(0xFFFE, 0x10001, 4), (0x10FF00, 0xFFFFFFFF, 6)], fmt=13))])]
    c["f12_id_passes_ffff_part_way"] = [face([(3, 10, fmt12([(0x10000, 0x1001F, 0xFFF0)]))])]
    c["f13_three_planes"] = [face([(0, 4, fmt12([(0x41, 0x42, 9), (0x10000, 0x10000, 4), (0x1FF00, 0x1FFFF, 6), (0x100000, 0x10FFFF, 7)], fmt=13))])]
    c["f10_first_in_plane_1"] = [face([(0, 4, fmt10(0x10020, [4, 0, 5, 6])), (0, 6, fmt10(0x1FFFE, [7, 9, 10]))])]
    c["f4_only"] = [plain_face(range(0x41, 0x60))]
    c["f4_in_front_of_f12"] = [face([(3, 1, fmt4([(0x41, 0x42, 0, [4, 5]), SENTINEL])), (3, 10, fmt12([(0x41, 0x42, 9), (0x10041, 0x10042, 10)]))])]
    c["two_faces_map_10400"] = [face([(3, 10, fmt12([(0x10400, 0x10401, 4)]))]), face([(3, 10, fmt12([(0x103FF, 0x10402, 7)]))], upm=2048)]
    c["past_id_in_plane_1_only"] = [face([(3, 10, fmt12([(0x41, 0x42, 4), (0x10041, 0x10041, PAST)]))])]
    pts = LANE_EDGES + [p + 0xF0000 for p in LANE_EDGES]
    c["lane_edges"] = [face([(3, 10, fmt12([(p, p, SMALL[i % len(SMALL)]) for i, p in enumerate(pts)]))])]
    # cmap_edge_tables' own tables with spans across U+FFFF: format 6 over 0xFFFE .. 0x10000 (a 16-bit format: nothing above),
    # format 10 from 0xFFFF, a format 12 group and a format 13 group across the edge
    regular = E.regular_cases()
    for name in ("format6", "format10", "format12", "format13"):
        c["bmp_" + name] = regular[name]
    return c


def census_cases():
    """tables for the census alone (their glyph ids do not matter)"""
    c = {}
    c["one_group_over_everything"] = [face([(3, 10, fmt12([(0, 0x10FFFF, 0)]))])]
    c["one_group_past_everything"] = [face([(3, 10, fmt12([(0, 0xFFFFFFFF, 0)], fmt=13))])]
    # one code point in the first and the last block of a word of the bitmap: words 0 | 1, and the last word
    c["word_ends"] = [face([(3, 10, fmt12([(0x0000, 0x0000, 1), (0x1FFF, 0x1FFF, 1), (0x2000, 0x2000, 1), (0x10E000, 0x10E000, 1), (0x10FFFF, 0x10FFFF, 1)]))])]
    c["whole_words"] = [face([(3, 10, fmt12([(0x1F80, 0x6010, 1), (0x20000, 0x3FFFF, 1)]))])]       # partial | full words | partial; aligned full words
    c["only_surrogates"] = [face([(3, 10, fmt12([(0xD800, 0xDFFF, 1)]))])]
    c["surrogates_and_one_more"] = [face([(3, 10, fmt12([(0xD7FF, 0xDFFF, 1)])), (3, 1, fmt4([(0xDFFF, 0xE000, 0, [4, 5]), SENTINEL]))])]
    c["format0"] = [face([(0, 0, E.fmt0({0x41: 6}))])]
    c["many_groups"] = [face([(3, 10, fmt12([(0x300 * k, 0x300 * k + k % 5, 1) for k in range(1, 700)]))])]     # more groups than lanes
    c["no_subtable"] = [face([])]
    return c
