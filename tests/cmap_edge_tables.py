"""What the tests of device-built family tables share (no test in here): hand-written `cmap` / `hmtx` tables at the edges of
the lookup, the face descriptions they make (vgsdf_face_tables), and a strict Python restatement of the table a family is:
for every code point of [0, 0xFFFF] outside the surrogates the first face that MAPS it (a unicode subtable enumerates it and that
subtable's lookup has a value), the first value any subtable of that face has, and advance, scale and shift_x in f64.

The restatement follows the host reader (ttf_face.cpp: CmapSubtable::glyph_index, for_each_codepoint, glyph_hor_advance;
renderer.cpp: record_resident) and is pinned to it by tests/test_family_tables_desc_host.py.  No tolerance appears anywhere."""
import math
import struct

import numpy as np

FORMATS = (0, 4, 6, 10, 12, 13)
# glyph ids that exist in the synthetic fonts of both kinds (family_ranges_kit) with a small outline / without one
SMALL = (4, 5, 6, 7, 9, 10, 11, 13, 14, 17)
EMPTY = (0, 8)
N_IDS = 20       # glyph ids below this exist in the synthetic fonts of both kinds
PAST = 23        # ... and this one in neither


def u16(b, o):
    return struct.unpack_from(">H", b, o)[0]


def u32(b, o):
    return struct.unpack_from(">I", b, o)[0]


# ---- the restatement ----

def is_unicode(platform, encoding, fmt):
    return platform == 0 or (platform == 3 and (encoding == 1 or (encoding == 10 and fmt in (12, 13))))


class _Sub:
    """a subtable: from its first byte to the end of the cmap table"""

    def __init__(self, cmap, off, fmt):
        self.d, self.fmt = bytes(cmap[off:]), int(fmt)

    def has(self, off, n):
        return off <= len(self.d) and n <= len(self.d) - off

    def _f4(self):
        d = self.d
        if not self.has(0, 14):
            return None
        x2 = u16(d, 6)
        if x2 < 2:
            return None
        segs = x2 // 2
        ends, starts = 14, 14 + segs * 2 + 2
        deltas, offsets = starts + segs * 2, starts + segs * 4
        return (segs, ends, starts, deltas, offsets) if self.has(offsets, segs * 2) else None

    def look(self, c):
        """CmapSubtable::glyph_index: a glyph id or None"""
        d, fmt = self.d, self.fmt
        if fmt == 0:
            if c >= 256 or not self.has(6, 256):
                return None
            return d[6 + c] or None
        if fmt == 4:
            t = self._f4()
            if t is None or c > 0xFFFF:
                return None
            segs, ends, starts, deltas, offsets = t
            lo, hi = 0, segs
            while lo < hi:
                mid = (lo + hi) // 2
                if u16(d, ends + mid * 2) < c:
                    lo = mid + 1
                    continue
                first = u16(d, starts + mid * 2)
                if first > c:
                    hi = mid
                    continue
                range_off, delta = u16(d, offsets + mid * 2), u16(d, deltas + mid * 2)
                if range_off == 0:
                    return (c + delta) & 0xFFFF
                if range_off == 0xFFFF:
                    return None
                twice = (c - first) * 2
                if twice > 0xFFFF:
                    return None
                pos = (((offsets + mid * 2) & 0xFFFF) + twice + range_off) & 0xFFFF
                if not self.has(pos, 2):
                    return None
                raw = u16(d, pos)
                if raw == 0:
                    return None
                gid = (raw + delta) & 0xFFFF
                return None if gid >= 0x8000 else gid
            return None
        if fmt == 6:
            if c > 0xFFFF or not self.has(0, 10):
                return None
            first, count = u16(d, 6), u16(d, 8)
            if c < first or c - first >= count or not self.has(10 + (c - first) * 2, 2):
                return None
            return u16(d, 10 + (c - first) * 2)
        if fmt == 10:
            if not self.has(0, 20):
                return None
            first, count = u32(d, 12), u32(d, 16)
            if c < first or c - first >= count or not self.has(20 + (c - first) * 2, 2):
                return None
            return u16(d, 20 + (c - first) * 2)
        if fmt in (12, 13):
            if not self.has(0, 16):
                return None
            n = u32(d, 12)
            if not self.has(16, n * 12):
                return None
            lo, hi = 0, n
            while lo < hi:
                mid = lo + (hi - lo) // 2
                g = 16 + mid * 12
                if u32(d, g) > c:
                    hi = mid
                elif u32(d, g + 4) < c:
                    lo = mid + 1
                else:
                    gid = u32(d, g + 8)
                    if fmt == 12:
                        gid += c
                        if gid > 0xFFFFFFFF:
                            return None
                        gid -= u32(d, g)
                    return None if gid > 0xFFFF else gid
            return None
        return None

    def listed(self):
        """for_each_codepoint, as inclusive ranges clipped to the BMP"""
        d, fmt, out = self.d, self.fmt, []
        if fmt == 0 and self.has(6, 256):
            out = [(c, c) for c in range(256) if d[6 + c]]
        elif fmt == 4 and self._f4() is not None:
            segs, ends, starts, _, _ = self._f4()
            for s in range(segs):
                a, b = u16(d, starts + s * 2), u16(d, ends + s * 2)
                if a == 0xFFFF and b == 0xFFFF:
                    break
                out.append((a, b))
        elif fmt == 6 and self.has(0, 10):
            out = [(u16(d, 6), u16(d, 6) + u16(d, 8) - 1)]
        elif fmt == 10 and self.has(0, 20):
            out = [(u32(d, 12), u32(d, 12) + u32(d, 16) - 1)]
        elif fmt in (12, 13) and self.has(0, 16) and self.has(16, u32(d, 12) * 12):
            out = [(u32(d, 16 + k * 12), u32(d, 20 + k * 12)) for k in range(u32(d, 12))]
        return [(a, min(b, 0xFFFF)) for a, b in out if a <= b and a <= 0xFFFF]


def hor_advance(t, gid):
    """Face::glyph_hor_advance(gid).value_or(0)"""
    hmtx, nh, ng = t["hmtx"], t["num_hmetrics"], t["num_glyphs"]
    if len(hmtx) == 0 or nh == 0 or ng == 0 or gid >= ng or len(hmtx) < nh * 4:
        return 0
    return u16(hmtx, 4 * min(gid, nh - 1))


def round_half_away(x):
    r = math.floor(x)
    return r + 1 if x - r >= 0.5 else r     # (x >= 0, x - r exact)


def varint_len(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def face_map(t):
    """{code point: glyph id} of one face description"""
    subs = [_Sub(t["cmap"], int(o), int(f)) for o, f in zip(t["subtable_off"], t["subtable_format"])]
    out = {}
    for s in subs:
        for a, b in s.listed():
            for c in range(a, b + 1):
                if c in out or 0xD800 <= c <= 0xDFFF or s.look(c) is None:
                    continue
                out[c] = next(g for g in (x.look(c) for x in subs) if g is not None)
    return out


def restate(faces):
    """the family of `faces` (descriptions, provider order) -> {code_point, font_of, glyph_id, advance, scale, shift_x, pbf_fix}"""
    owner = {}
    for k, t in enumerate(faces):
        for c, g in face_map(t).items():
            owner.setdefault(c, (k, g))
    cps = sorted(owner)
    font_of, gid, adv, scale, shift, fix = [], [], [], [], [], []
    for c in cps:
        k, g = owner[c]
        t = faces[k]
        s = 24.0 / float(t["units_per_em"])
        af = float(hor_advance(t, g)) * s * 0.95
        a = round_half_away(af)
        font_of.append(k), gid.append(g), adv.append(a), scale.append(s), shift.append((float(a) - af) / 2.0)
        fix.append((1 + varint_len(c)) | ((1 + varint_len(a)) << 4))
    return {"code_point": np.array(cps, np.uint16), "font_of": np.array(font_of, np.uint16), "glyph_id": np.array(gid, np.uint16),
            "advance": np.array(adv, np.uint32), "scale": np.array(scale, np.float64), "shift_x": np.array(shift, np.float64),
            "pbf_fix": np.array(fix, np.uint8)}


# ---- builders ----

def fmt0(mapping):
    g = bytearray(256)
    for c, v in mapping.items():
        g[c] = v
    return struct.pack(">HHH", 0, 262, 0) + bytes(g)


def fmt4(segs, language=0, tail=b""):
    """segs: (start, end, delta, how); how: 0 / 0xFFFF / another int = that idRangeOffset as it stands, a list = the segment's raw
    glyph array (its idRangeOffset is worked out), ("at", p) = the offset that makes the segment's first position p (mod 65536)"""
    n = len(segs)
    offsets_at = 14 + n * 2 + 2 + n * 4
    array_at = offsets_at + n * 2
    array, offs = [], []
    for k, (a, b, delta, how) in enumerate(segs):
        here = offsets_at + 2 * k
        if isinstance(how, list):
            offs.append(array_at + 2 * len(array) - here)
            array += how
        elif isinstance(how, tuple):
            offs.append((how[1] - here) & 0xFFFF)
        else:
            offs.append(how)
    body = b"".join(struct.pack(">H", s[1]) for s in segs) + b"\0\0" + b"".join(struct.pack(">H", s[0]) for s in segs)
    body += b"".join(struct.pack(">H", s[2] & 0xFFFF) for s in segs) + b"".join(struct.pack(">H", o & 0xFFFF) for o in offs)
    body += b"".join(struct.pack(">H", v) for v in array) + tail
    return struct.pack(">HHHHHHH", 4, (14 + len(body)) & 0xFFFF, language, 2 * n, 0, 0, 0) + body


SENTINEL = (0xFFFF, 0xFFFF, 1, 0)    # as in every fixture font: glyph_index(0xFFFF) is Some(0), the code point is not listed


def fmt6(first, gids):
    return struct.pack(">HHHHH", 6, 10 + 2 * len(gids), 0, first, len(gids)) + b"".join(struct.pack(">H", g) for g in gids)


def fmt10(first, gids):
    return struct.pack(">HHIIII", 10, 0, 20 + 2 * len(gids), 0, first, len(gids)) + b"".join(struct.pack(">H", g) for g in gids)


def fmt12(groups, fmt=12, n=None):
    return struct.pack(">HHIII", fmt, 0, 16 + 12 * len(groups), 0, len(groups) if n is None else n) + \
        b"".join(struct.pack(">III", *g) for g in groups)


def fmt_other(fmt):
    """a record of format 2 or 14: never a value"""
    return struct.pack(">HH", fmt, 64) + bytes(60) if fmt == 2 else struct.pack(">HII", 14, 10, 0)


def cmap_table(records):
    """records: (platform, encoding, subtable bytes) in record order -> the table; the subtables follow in that order"""
    at, head, body = 4 + 8 * len(records), b"", b""
    for p, e, sub in records:
        head += struct.pack(">HHI", p, e, at + len(body))
        body += sub
    return struct.pack(">HH", 0, len(records)) + head + body


def hmtx_table(advances, n_glyphs=None):
    n = len(advances) if n_glyphs is None else n_glyphs
    return b"".join(struct.pack(">Hh", a, 0) for a in advances) + bytes(2 * max(n - len(advances), 0))


def face(records, advances=None, upm=1000, num_glyphs=N_IDS, num_hmetrics=None, hmtx=None):
    """a face: its tables and counts, and `records` for the tests that splice it into a font file"""
    advances = [500 + 37 * g for g in range(num_glyphs)] if advances is None else advances
    return {"records": records, "cmap": cmap_table(records), "hmtx": hmtx_table(advances, num_glyphs) if hmtx is None else hmtx,
            "units_per_em": upm, "num_glyphs": num_glyphs, "num_hmetrics": len(advances) if num_hmetrics is None else num_hmetrics}


def describe(f):
    """vg_manager_family_tables_desc of such a face: the records, in order, that are unicode and of a format the lookup knows"""
    cmap, off, fmt = f["cmap"], [], []
    for i in range(u16(cmap, 2)):
        p, e, o = u16(cmap, 4 + 8 * i), u16(cmap, 6 + 8 * i), u32(cmap, 8 + 8 * i)
        if o + 2 > len(cmap):
            continue
        fm = u16(cmap, o)
        if is_unicode(p, e, fm) and fm in FORMATS:
            off.append(o), fmt.append(fm)
    return {"cmap": cmap, "hmtx": f["hmtx"], "units_per_em": f["units_per_em"], "num_glyphs": f["num_glyphs"], "num_hmetrics": f["num_hmetrics"],
            "subtable_off": np.array(off, np.uint32), "subtable_format": np.array(fmt, np.uint16)}


def runs_of(cps):
    cps = sorted(cps)
    out = []
    for c in cps:
        if out and out[-1][1] == c - 1:
            out[-1][1] = c
        else:
            out.append([c, c])
    return out


def plain_face(cps, gids=SMALL, sentinel=True, **kw):
    """format 4 over the runs of `cps`, glyph ids from `gids` in turn through glyph arrays"""
    segs, i = [], 0
    for a, b in runs_of(cps):
        segs.append((a, b, 0, [gids[(i + j) % len(gids)] for j in range(b - a + 1)]))
        i += b - a + 1
    if sentinel and not (segs and segs[-1][1] == 0xFFFF):
        segs.append(SENTINEL)
    return face([(3, 1, fmt4(segs))], **kw)


def _seg_count_face(n):
    """n segments, the last one the closing one"""
    segs = [(0x100 * (k + 1), 0x100 * (k + 1) + k % 3, 0, [SMALL[(k + j) % len(SMALL)] for j in range(k % 3 + 1)]) for k in range(n - 1)]
    return face([(3, 1, fmt4(segs + [SENTINEL]))])


def _range_offset_face():
    """one segment per exit of the idRangeOffset branch; the subtable is the cmap's last, so its end is the table's"""
    tail = struct.pack(">H", 11)

    def segs(sub_len):
        return [
            (0x20, 0x22, 0, [4, 0, 5]),                                # raw 0 in the middle: no value
            (0x30, 0x31, 0x15, [0xFFF0, 0xFFF1]),                      # raw + delta wraps: 5, 6
            (0x40, 0x41, 5, [0x7FFF, 2]),                              # 0x8004 is negative as i16: no value; 7
            (0x50, 0x51, 3, 0xFFFF),                                   # idRangeOffset 0xFFFF: no value
            (0x60, 0x60, 0, ("at", 0x10000 + 4)),                      # the position wraps in u16 onto the language field: 9
            (0x80, 0x80, 0, ("at", sub_len - 2)),                      # the table's last two bytes: 11
            (0x90, 0x90, 0, ("at", sub_len - 1)),                      # one byte further: not inside
            (0xF070, 0xF071, (SMALL[2] - 0xF070) & 0xFFFF, 0),         # idDelta wraps mod 65536: SMALL[2] and the next id
            SENTINEL,
        ]
    sub_len = len(fmt4(segs(0), tail=tail))
    return face([(3, 1, fmt4(segs(sub_len), language=9, tail=tail))])


def _several_faces(n_faces):
    base = list(range(0x41, 0x41 + 40))
    sets = [base[::2], base[5:15], base + [0x3000, 0x3001]][:n_faces]     # a later face maps a subset, a superset
    return [plain_face(s, gids=SMALL[k:] + SMALL[:k], upm=(1000, 2048, 512)[k]) for k, s in enumerate(sets)]


def regular_cases():
    """name -> faces (provider order) of regular tables: what the device builds and the host reader answers alike"""
    c = {}
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        c[f"entries_{n}"] = [plain_face([0x21 + 3 * (i // 2) + (i % 2) for i in range(n)])]
    c["workgroups"] = [plain_face(list(range(0x300, 0x400)) + [0x500, 0x6FF, 0x4000, 0xF0FF])]
    c["special_code_points"] = [plain_face([0] + list(range(0xD7FF, 0xE001)) + [0xFFFE])]
    c["ffff_listed"] = [plain_face(list(range(0xFFF0, 0x10000)))]
    for n in (1, 2, 3, 4, 5, 64):
        c[f"format4_{n}_segments"] = [_seg_count_face(n)]
    c["format4_range_offsets"] = [_range_offset_face()]
    c["format12"] = [face([(3, 10, fmt12([(0x41, 0x41, 7), (0x100, 0x103, 0x10000), (0x200, 0x201, 0xFFFFFFFF), (0x300, 0x304, 9),
                                         (0xFFF0, 0x1000F, 4)]))])]
    c["format13"] = [face([(0, 4, fmt12([(0x41, 0x50, 6), (0x60, 0x60, 0x10000), (0xFFFE, 0x20000, 5)], fmt=13))])]
    c["format0"] = [face([(0, 0, fmt0({0: 5, 0x41: 6, 255: 7}))])]
    c["format6"] = [face([(0, 3, fmt6(0x41, [4, 0, 5])), (3, 1, fmt6(0xFFFE, [6, 7, 9]))])]
    c["format10"] = [face([(0, 4, fmt10(0x2000, [4, 5])), (0, 6, fmt10(0xFFFF, [6, 7]))])]
    c["skipped_records"] = [face([(1, 0, fmt0({0x41: 4})), (3, 0, fmt4([(0x41, 0x42, 0, [5, 6]), SENTINEL])), (0, 5, fmt_other(14)),
                                  (0, 3, fmt_other(2)), (3, 10, fmt4([(0x43, 0x43, 0, [7]), SENTINEL])), (3, 1, fmt4([(0x44, 0x45, 0, [9, 10]), SENTINEL]))])]
    # the first subtable has a value at 0xFFFF (its closing segment: glyph 0) and does not list it, the second lists it; and a
    # code point only the second has
    c["two_subtables"] = [face([(3, 1, fmt4([(0x41, 0x42, 0, [4, 5]), SENTINEL])), (3, 10, fmt12([(0x43, 0x43, 6), (0xFFFF, 0xFFFF, 7)]))])]
    adv = [300, 0, 65535, 127, 128] + [400 + g for g in range(5, N_IDS)]     # (glyph id 0 is "no value" in a glyph array)
    cps = list(range(0x41, 0x41 + N_IDS))
    every = list(range(N_IDS))
    c["hmtx_one_metric"] = [plain_face(cps, gids=every, advances=[777], num_glyphs=N_IDS)]
    c["hmtx_all_metrics"] = [plain_face(cps, gids=every, advances=adv)]
    c["hmtx_tail"] = [plain_face(cps, gids=every, advances=adv[:6], num_glyphs=N_IDS)]
    c["hmtx_few_glyphs"] = [plain_face(cps, gids=every, advances=adv[:5], num_glyphs=5)]
    c["hmtx_short"] = [plain_face(cps, gids=every, hmtx=hmtx_table(adv)[:4 * N_IDS - 1], num_hmetrics=N_IDS)]
    c["hmtx_empty"] = [plain_face(cps, gids=every, hmtx=b"", num_hmetrics=N_IDS)]
    for upm in (16, 1000, 2048, 16384):
        c[f"upm_{upm}"] = [plain_face(cps, gids=every, advances=adv, upm=upm)]
    c["half_boundary"] = [plain_face(cps, gids=every, advances=[20, 100, 300, 500, 1] + adv[5:], upm=16)]
    # every step of a varint's length: code points, and advances 127 / 128 (24 / 2280 * 0.95 is 0.01)
    c["varint_steps"] = [plain_face([0x7F, 0x80, 0x3FFF, 0x4000], gids=(4, 5, 6, 7), advances=[0, 0, 0, 0, 12700, 12800, 12749, 12751] + [0] * 12, upm=2280)]
    for n in (1, 2, 3):
        c[f"faces_{n}"] = _several_faces(n)
    c["middle_face_maps_nothing"] = [_several_faces(1)[0], face([(3, 1, fmt4([SENTINEL]))]), face([]), _several_faces(3)[2]]
    return c


def past_case():
    """a code point mapped to a glyph id neither synthetic font has"""
    return [plain_face([0x41, 0x42, 0x43], gids=(4, PAST, 5))]


def irregular_cases():
    """name -> one face whose description REFUSES, while the host reader still answers"""
    ok = (0x41, 0x45, 0, [4, 5, 6, 7, 9])
    return {
        "format4_overlap": face([(3, 1, fmt4([ok, (0x45, 0x48, 0, [4, 5, 6, 7]), SENTINEL]))]),
        "format4_descending": face([(3, 1, fmt4([(0x60, 0x61, 0, [4, 5]), ok, SENTINEL]))]),
        "format4_start_above_end": face([(3, 1, fmt4([ok, (0x52, 0x50, 0, [4]), SENTINEL]))]),
        "format4_no_segments": face([(3, 1, struct.pack(">HHHHHHH", 4, 16, 0, 0, 0, 0, 0) + bytes(8)), (3, 10, fmt12([(0x41, 0x42, 4)]))]),
        "format4_arrays_outside": face([(3, 10, fmt12([(0x41, 0x42, 4)])), (3, 1, struct.pack(">HHHHHHH", 4, 16, 0, 400, 0, 0, 0) + bytes(8))]),
        "format12_overlap": face([(3, 10, fmt12([(0x41, 0x45, 4), (0x45, 0x46, 5)]))]),
        "format12_descending": face([(3, 10, fmt12([(0x61, 0x62, 4), (0x41, 0x42, 5)]))]),
        "format12_start_above_end": face([(3, 10, fmt12([(0x41, 0x42, 4), (0x52, 0x50, 5)]))]),
        "format12_groups_outside": face([(3, 1, fmt4([ok, SENTINEL])), (3, 10, fmt12([(0x41, 0x42, 4)], n=9))]),
    }
