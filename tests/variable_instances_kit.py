"""Fixtures and strict restatements for the tests of variable-font instances (a CFF2 file rendered at a chosen position of its
design space, advances from `HVAR`).  No tests here.

The fixtures are built with fontTools from Fira Sans' outlines, as tests/test_cff2_outlines.py builds its variable font, but
with masters whose ADVANCES differ, so that `HVAR` matters.  The restatements (normalize, avar_map, axis_factor,
region_scalars, hvar_advance) are written from the rules R1-R5 the readers state in csrc/host/ttf_face.hpp, cff.hpp and
include/vgsdf.h, in numpy float32 / Python integers, and not from the C++.  yardstick_files builds the PBF files of an instance
without the product's reader: fontTools' outlines and widths at the location, the reference's arithmetic in f64, the oracle's
ring builder, raster and encoder.
"""
import io
import math
import struct

import numpy as np

from conftest import FIRA

from fontTools.fontBuilder import FontBuilder
from fontTools.ttLib import TTFont, newTable

f32 = np.float32
BOLD = (1.25, 0, 0.1, 1.05, 7, -3)          # the second master's transform (tests/test_cff2_outlines.py)
CONDENSED, WIDE = (0.75, 0, 0, 1, 0, 0), (1.5, 0, 0, 1.0, 4, 0)
# positions at which every coordinate and every width fontTools interpolates is exact in f32 (normalised 0.25, 0.5, 1)
EXACT_ONE_AXIS = [{"wght": 525}, {"wght": 650}, {"wght": 900}]
EXACT_TWO_AXES = {"wght": 650, "wdth": 150}

_CACHE = {}


def variable_fira(n_glyphs=120, two_axes=False, avar=None):
    """masters of Fira Sans outlines merged by fontTools.varLib into a CFF2 font with fvar, HVAR (advance-width map, mixed
    i16 / i8 columns) and two named instances; the second master's advances are int(width * 1.25) + 4 * (i mod 3).
    two_axes: `wdth` 50 / 100 / 200 with a condensed and a wide master.  avar: {tag: {from: to}} in normalised values"""
    key = (n_glyphs, two_axes, repr(avar))
    if key in _CACHE:
        return _CACHE[key]
    from fontTools import varLib
    from fontTools.designspaceLib import AxisDescriptor, DesignSpaceDocument, SourceDescriptor
    from fontTools.pens.t2CharStringPen import T2CharStringPen
    from fontTools.pens.transformPen import TransformPen
    from fontTools.ttLib.tables._f_v_a_r import NamedInstance
    src = TTFont(FIRA)
    gs = src.getGlyphSet()
    order = src.getGlyphOrder()[:n_glyphs]
    cmap = {cp: g for cp, g in src.getBestCmap().items() if g in order}

    def master(xform, style, width_of):
        fb = FontBuilder(src["head"].unitsPerEm, isTTF=False)
        fb.setupGlyphOrder(order)
        fb.setupCharacterMap(cmap)
        cs = {}
        for g in order:
            pen = T2CharStringPen(gs[g].width, gs)
            gs[g].draw(TransformPen(pen, xform))
            # (two axes: unspecialised programs — a pure horizontal scale rounds some short curves of one master to lines, and
            # varLib merges point types, not shapes)
            cs[g] = pen.getCharString(optimize=not two_axes)
        fb.setupCFF("SynthVar-" + style, {"FullName": "Synth Var " + style}, cs, {})
        fb.setupHorizontalMetrics({g: (width_of(i, gs[g].width), 0) for i, g in enumerate(order)})
        fb.setupHorizontalHeader(ascent=935, descent=-265)
        fb.setupNameTable({"familyName": "Synth Var", "styleName": style})
        fb.setupOS2()
        fb.setupPost()
        buf = io.BytesIO()
        fb.save(buf)
        return TTFont(io.BytesIO(buf.getvalue()))

    ds = DesignSpaceDocument()
    a = AxisDescriptor()
    a.tag, a.name, a.minimum, a.default, a.maximum = "wght", "Weight", 400, 400, 900
    ds.addAxis(a)
    if two_axes:
        a = AxisDescriptor()
        a.tag, a.name, a.minimum, a.default, a.maximum = "wdth", "Width", 50, 100, 200
        ds.addAxis(a)
    masters = [(master((1, 0, 0, 1, 0, 0), "Regular", lambda i, w: w), {"Weight": 400}),
               (master(BOLD, "Bold", lambda i, w: int(w * 1.25) + 4 * (i % 3)), {"Weight": 900})]
    if two_axes:
        for m, loc in masters:
            loc["Width"] = 100
        masters += [(master(CONDENSED, "Condensed", lambda i, w: int(w * 0.75) + (i % 2)), {"Weight": 400, "Width": 50}),
                    (master(WIDE, "Wide", lambda i, w: int(w * 1.5) + 2 * (i % 5)), {"Weight": 400, "Width": 200})]
    for font, loc in masters:
        s = SourceDescriptor()
        s.font, s.location, s.familyName, s.styleName = font, loc, "Synth Var", "x"
        ds.addSource(s)
    vf, _, _ = varLib.build(ds, optimize=True)
    for name_id, coords in ((2, {"wght": 400}), (17, {"wght": 650})):
        ni = NamedInstance()
        ni.subfamilyNameID, ni.flags = name_id, 0
        ni.coordinates = dict(coords, **({"wdth": 100 + (name_id == 17) * 50} if two_axes else {}))
        vf["fvar"].instances.append(ni)
    if avar:
        t = newTable("avar")
        t.majorVersion, t.minorVersion = 1, 0
        t.segments = {ax.axisTag: dict(avar.get(ax.axisTag, {-1.0: -1.0, 0.0: 0.0, 1.0: 1.0})) for ax in vf["fvar"].axes}
        vf["avar"] = t
    buf = io.BytesIO()
    vf.save(buf)
    _CACHE[key] = buf.getvalue()
    return _CACHE[key]


# ---- restatements -------------------------------------------------------------------------------------------------------------

def normalize(v, lo, de, hi):
    """R1: a user-space value -> F2Dot14, all in float32, truncated toward zero"""
    v, lo, de, hi = f32(v), f32(lo), f32(de), f32(hi)
    v = min(max(v, lo), hi)
    if v == de:
        n = f32(0)
    elif v < de:
        n = f32(v - de) / f32(de - lo)
    else:
        n = f32(v - de) / f32(hi - de)
    n = min(max(n, f32(-1)), f32(1))
    return int(math.trunc(float(f32(n * f32(16384)))))


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def avar_map(v, pairs):
    """R2: one axis' segment map [(from, to)] (F2Dot14 integers) applied to v, truncating division"""
    if not pairs:
        return v
    fr, to = [p[0] for p in pairs], [p[1] for p in pairs]
    if len(pairs) == 1:
        r = v - fr[0] + to[0]
    elif v <= fr[0]:
        r = v - fr[0] + to[0]
    else:
        i = next((k for k in range(1, len(pairs)) if v <= fr[k]), len(pairs) - 1)
        if v >= fr[i]:
            r = v - fr[i] + to[i]
        elif fr[i - 1] == fr[i]:
            r = to[i - 1]
        else:
            d = fr[i] - fr[i - 1]
            r = to[i - 1] + _tdiv((to[i] - to[i - 1]) * (v - fr[i - 1]) + _tdiv(d, 2), d)
    return r if -32768 <= r <= 32767 else v


def _table(font_bytes, tag):
    """a table's raw bytes from the file's directory (no fontTools parser in the way)"""
    n = struct.unpack(">H", font_bytes[4:6])[0]
    for i in range(n):
        rec = font_bytes[12 + 16 * i:28 + 16 * i]
        if rec[:4] == tag.encode():
            off, ln = struct.unpack(">II", rec[8:16])
            return font_bytes[off:off + ln]
    return None


def fvar_axes(font_bytes):
    """[(tag, min, default, max)] read from the raw fvar"""
    t = _table(font_bytes, "fvar")
    at, n = struct.unpack(">H", t[4:6])[0], struct.unpack(">H", t[8:10])[0]
    return [(t[at + 20 * i:at + 20 * i + 4].decode(),) + tuple(v / 65536.0 for v in struct.unpack(">iii", t[at + 20 * i + 4:at + 20 * i + 16]))
            for i in range(n)]


def avar_maps(font_bytes):
    t = _table(font_bytes, "avar")
    if t is None or struct.unpack(">I", t[:4])[0] != 0x00010000:
        return None
    n_axes, at, maps = struct.unpack(">H", t[6:8])[0], 8, []
    for _ in range(n_axes):
        n = struct.unpack(">H", t[at:at + 2])[0]
        maps.append([struct.unpack(">hh", t[at + 2 + 4 * k:at + 6 + 4 * k]) for k in range(n)])
        at += 2 + 4 * n
    return maps


def with_raw_avar(font_bytes, maps, version=0x00010000):
    """the font with an avar table written byte by byte: maps = per axis [(from, to)] in F2Dot14 integers, as they stand (fontTools'
    compiler would insist on the -1 / 0 / 1 records)"""
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    raw = DefaultTable("avar")
    raw.data = struct.pack(">IHH", version, 0, len(maps)) + b"".join(
        struct.pack(">H", len(m)) + b"".join(struct.pack(">hh", a, b) for a, b in m) for m in maps)
    font = TTFont(io.BytesIO(font_bytes), recalcBBoxes=False, recalcTimestamp=False)
    font["avar"] = raw
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


def coords_of(font_bytes, location):
    """user space -> the final normalised coordinates (R1 then R2), axes not named at their default"""
    axes = fvar_axes(font_bytes)
    coords = [normalize(location[t], lo, de, hi) if t in location else 0 for t, lo, de, hi in axes]
    maps = avar_maps(font_bytes)
    if maps is not None and len(maps) == len(coords):
        coords = [avar_map(c, m) for c, m in zip(coords, maps)]
    return coords


def axis_factor(coord, start, peak, end):
    """R3, one axis: int16 inputs, a float32 result from ONE float32 divide"""
    if start > peak or peak > end:
        return f32(1)
    if start < 0 and end > 0 and peak != 0:
        return f32(1)
    if peak == 0 or coord == peak:
        return f32(1)
    if coord <= start or coord >= end:
        return f32(0)
    if coord < peak:
        return f32(coord - start) / f32(peak - start)
    return f32(end - coord) / f32(end - peak)


def region_scalars(region_list, coords):
    """R3: the factor of every region of a VariationRegionList (bytes from axisCount on) at coords; the record index is kept in
    16 bits as the readers keep it"""
    n_axes, n_regions = struct.unpack(">HH", region_list[:4])
    out = []
    for r in range(n_regions):
        v = f32(1)
        for i, c in enumerate(coords):
            rec = r * n_axes + i
            if r * n_axes > 0xFFFF or rec > 0xFFFF or rec >= n_axes * n_regions:
                v = f32(0)
                break
            s, p, e = struct.unpack(">hhh", region_list[4 + 6 * rec:10 + 6 * rec])
            f = axis_factor(c, s, p, e)
            if f == 0:
                v = f32(0)
                break
            v = f32(v * f)
        out.append(v)
    return np.array(out, f32)


def hvar_parts(hvar):
    """(store offset, map offset, region list bytes) of an HVAR table"""
    store, amap = struct.unpack(">II", hvar[4:12])
    regions_at = struct.unpack(">I", hvar[store + 2:store + 6])[0]
    return store, amap, hvar[store + regions_at:]


def hvar_delta(hvar, gid, scalars):
    """R4: the offset of glyph gid's advance (float32), or None"""
    n = len(hvar)
    store, amap, _ = hvar_parts(hvar)
    outer, inner = 0, gid
    if amap:
        if amap + 2 > n:
            return None
        fmt, ef = hvar[amap], hvar[amap + 1]
        if fmt > 1 or amap + 2 + (4 if fmt else 2) > n:
            return None
        count = struct.unpack(">I", hvar[amap + 2:amap + 6])[0] if fmt else struct.unpack(">H", hvar[amap + 2:amap + 4])[0]
        if count == 0:
            return None
        size = ((ef >> 4) & 3) + 1
        at = amap + (6 if fmt else 4) + size * min(gid, count - 1)
        if at + size > n:
            return None
        entry = int.from_bytes(hvar[at:at + size], "big")
        bits = (ef & 15) + 1
        outer, inner = entry >> bits, entry & ((1 << bits) - 1)
        if outer > 0xFFFF:
            return None
    n_data = struct.unpack(">H", hvar[store + 6:store + 8])[0]
    if outer >= n_data:
        return None
    at = store + struct.unpack(">I", hvar[store + 8 + 4 * outer:store + 12 + 4 * outer])[0]
    if at + 6 > n:
        return None
    items, words, cols = struct.unpack(">HHH", hvar[at:at + 6])
    if at + 6 + 2 * cols > n or inner >= items or words > cols:
        return None
    row = at + 6 + 2 * cols + inner * (words + cols)
    if row + words + cols > n:
        return None
    d, p = f32(0), row
    for c in range(cols):
        region = struct.unpack(">H", hvar[at + 6 + 2 * c:at + 8 + 2 * c])[0]
        if c < words:
            num, p = struct.unpack(">h", hvar[p:p + 2])[0], p + 2
        else:
            num, p = struct.unpack(">b", hvar[p:p + 1])[0], p + 1
        fac = scalars[region] if region < len(scalars) else f32(0)
        d = f32(d + f32(f32(num) * fac))
    return d


def hvar_advance(font_bytes, gid, coords):
    """R5: the advance of glyph gid of a face at `coords` (None: a static face, the hmtx advance alone)"""
    hmtx, hhea, maxp = _table(font_bytes, "hmtx"), _table(font_bytes, "hhea"), _table(font_bytes, "maxp")
    n_h, n_g = struct.unpack(">H", hhea[34:36])[0], struct.unpack(">H", maxp[4:6])[0]
    if gid >= n_g or n_h == 0:
        return 0
    adv = struct.unpack(">H", hmtx[4 * min(gid, n_h - 1):4 * min(gid, n_h - 1) + 2])[0]
    hvar = _table(font_bytes, "HVAR")
    if coords is None or hvar is None:
        return adv
    a = f32(adv)
    d = hvar_delta(hvar, gid, region_scalars(hvar_parts(hvar)[2], coords))
    if d is not None:
        a = f32(a + f32(d + f32(0.5)))
    v = int(math.trunc(float(a)))
    return v if 0 <= v <= 65535 else 0


def family_entries(faces):
    """the family table of `faces` = [(font bytes, coords or None)] in provider order, as the host states it: code point ->
    (face, glyph id, advance, scale, shift_x) in the arithmetic of Renderer::record_resident (f64)"""
    taken, rows = set(), []
    for k, (fb, coords) in enumerate(faces):
        f = TTFont(io.BytesIO(fb), lazy=True)
        upem = f["head"].unitsPerEm
        for cp, name in sorted(f.getBestCmap().items()):
            if cp > 0xFFFF or cp in taken:
                continue
            taken.add(cp)
            gid = f.getGlyphID(name)
            scale = 24.0 / upem
            adv_f = float(hvar_advance(fb, gid, coords)) * scale * 0.95
            adv = int(math.floor(adv_f + 0.5)) if adv_f >= 0 else 0
            rows.append((cp, k, gid, adv, scale, (adv - adv_f) / 2.0))
    rows.sort()
    return {"code_point": np.array([r[0] for r in rows], np.uint16), "font_of": np.array([r[1] for r in rows], np.uint16),
            "glyph_id": np.array([r[2] for r in rows], np.uint16), "advance": np.array([r[3] for r in rows], np.uint32),
            "scale": np.array([r[4] for r in rows], np.float64), "shift_x": np.array([r[5] for r in rows], np.float64)}


# ---- HVAR tables by hand --------------------------------------------------------------------------------------------------

def _hvar(regions, datas, amap=None, words_flag=0, pad_rows=True, trailing=b""):
    """regions: [(start, peak, end)] of one axis; datas: [(item rows [[deltas]], word count, region indices)]; amap: None or
    (format, entry format, [entries]) -> an HVAR table with the store at 20 and the map behind it"""
    rl = struct.pack(">HH", 1, len(regions)) + b"".join(struct.pack(">hhh", *r) for r in regions)
    head = 8 + 4 * len(datas)
    body, offs = rl, []
    for rows, words, idx in datas:
        offs.append(head + len(body))
        b = struct.pack(">HHH", len(rows), words | words_flag, len(idx)) + b"".join(struct.pack(">H", i) for i in idx)
        for row in rows:
            b += b"".join(struct.pack(">h" if c < words else ">b", v) for c, v in enumerate(row))
        body += b
    store = struct.pack(">HIH", 1, head, len(datas)) + b"".join(struct.pack(">I", o) for o in offs) + body
    m = b""
    if amap is not None:
        fmt, ef, entries = amap
        size = ((ef >> 4) & 3) + 1
        m = struct.pack(">BB", fmt, ef) + (struct.pack(">I", len(entries)) if fmt else struct.pack(">H", len(entries)))
        m += b"".join(int(e).to_bytes(size, "big") for e in entries)
    return struct.pack(">HHIIII", 1, 0, 20, (20 + len(store)) if amap is not None else 0, 0, 0) + store + m + trailing


def _with_hvar(base, hvar, advances=None):
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    font = TTFont(io.BytesIO(base), recalcBBoxes=False, recalcTimestamp=False)
    if advances:
        for g, a in advances.items():
            font["hmtx"].metrics[font.getGlyphName(g)] = (a, 0)
    raw = DefaultTable("HVAR")
    raw.data = hvar
    font["HVAR"] = raw
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


def _entry(outer, inner, bits):
    return (outer << bits) | inner


def hvar_edge_faces():
    """{case: (font bytes, refused at parse, refused by the device description)}: small CFF2 faces (sized_face(64) of
    tests/charstring2_edge_programs.py: one axis `wght`, hmtx 600 throughout) whose HVAR is written by hand, one face per case"""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    import charstring2_edge_programs as E
    face = E.sized_face(64)
    base, n = face.font(), len(face.glyphs)
    assert n <= 70, n
    regions = [(0, 16384, 16384), (0, 8192, 16384), (-16384, -16384, 0)]      # factors at 0.5: 0.5, 1, 0; at 1: 1, 0, 0
    rows = [[(7 * g) % 300 - 150, (11 * g) % 200 - 100, g % 100 - 50] for g in range(n)]
    direct = (rows, 1, [0, 1, 2])
    small = ([[300 + i, -i, i] for i in range(4)], 2, [1, 0, 2])
    out = {}

    def add(case, hvar, refused=False, desc_refused=False, advances=None):
        out[case] = (_with_hvar(base, hvar, advances), refused, desc_refused)

    add("no_map", _hvar(regions, [direct]))
    for fmt in (0, 1):
        for size, bits in ((1, 4), (2, 8), (3, 16), (4, 16), (1, 1)):
            ent = [_entry(g % 2, (g * 3) % (n if g % 2 == 0 else 4) & ((1 << bits) - 1), bits) for g in range(n)]
            add(f"map{fmt}_size{size}_bits{bits}", _hvar(regions, [direct, small], (fmt, ((size - 1) << 4) | (bits - 1), ent)))
    add("map_short", _hvar(regions, [direct, small], (0, 0x17, [_entry(1, 2, 8), _entry(0, 5, 8), _entry(1, 3, 8)])))   # glyph ids past 2 clamp
    add("map_empty", _hvar(regions, [direct], (0, 0x17, [])))
    add("inner_at_count", _hvar(regions, [direct, small], (0, 0x17, [_entry(1, 3, 8), _entry(1, 4, 8), _entry(1, 5, 8), _entry(0, n, 8)])))
    add("outer_past", _hvar(regions, [direct, small], (0, 0x17, [_entry(1, 1, 8), _entry(2, 0, 8), _entry(200, 0, 8)])))
    add("words0", _hvar(regions, [([[g % 100 - 50, (3 * g) % 90 - 45, 5] for g in range(n)], 0, [0, 1, 2])]))
    add("words_all", _hvar(regions, [([[300 * (g % 7) - 900, 1000 - g, -129] for g in range(n)], 3, [0, 1, 2])]))
    add("region_past", _hvar(regions, [([[50 + g, 60, 70] for g in range(n)], 1, [0, 7, 1])]))
    add("zero_regions", _hvar([], [([[] for _ in range(n)], 0, [])]))
    add("zero_columns", _hvar(regions, [([[] for _ in range(n)], 0, [])]))
    short = _hvar(regions, [direct])
    add("row_past_table", short[:len(short) - 5 * 4 - 2])                               # the last rows leave the table
    add("below_zero_above_u16", _hvar(regions, [([[-700 if g % 2 else 32767, -100 if g % 2 else 32767, 0] for g in range(n)], 2, [0, 1, 2])]),
        advances={g: 65000 for g in range(0, n, 4)})
    add("long_words", _hvar(regions, [direct], words_flag=0x8000), refused=True)
    add("map_format2", _hvar(regions, [direct], (2, 0x17, [_entry(0, g, 8) for g in range(n)])), desc_refused=True)
    add("words_past_columns", _hvar(regions, [([[1, 2, 3]] * n, 3, [0, 1])]), desc_refused=True)
    _CACHE["edge"] = out
    return out


EDGE_POSITIONS = ([16384], [8192], [-8192])     # (the third: the region on the negative side has factor 0.5)


# ---- the independent yardstick -------------------------------------------------------------------------------------------

def fonttools_instance(font_bytes, location):
    """({cp: callbacks}, {cp: width}) of fontTools' glyph set at `location`; asserts that every coordinate and width is exact in
    float32 and a multiple of 1/8 (the positions the yardstick is valid at)"""
    from test_cff2_outlines import _fonttools_callbacks
    f = TTFont(io.BytesIO(font_bytes))
    full = {a.axisTag: location.get(a.axisTag, a.defaultValue) for a in f["fvar"].axes}
    gs, cmap = f.getGlyphSet(location=full), f.getBestCmap()
    widths = {cp: gs[name].width for cp, name in cmap.items()}
    for w in widths.values():
        assert w * 8 == int(w * 8), w
    # (the callbacks are rounded to float32 by _fonttools_callbacks: compare with the doubles once more)
    from fontTools.pens.recordingPen import RecordingPen
    for cp, name in cmap.items():
        rp = RecordingPen()
        gs[name].draw(rp)
        for _, args in rp.value:
            for pt in args:
                for v in pt:
                    assert v * 8 == int(v * 8) and abs(v) < 1 << 20, (hex(cp), v)
    return _fonttools_callbacks(font_bytes, location=full), widths


def yardstick_files(font_bytes, location, name, oracle, mode=None):
    """{path: bytes} of the instance of font_bytes at `location` under font id `name`, without the product: fontTools'
    callbacks and widths, advance = floor(width + 0.5), the arithmetic of the reference's render_glyph in f64, the oracle's
    rings, raster and encoder"""
    mode = oracle.PRECISE if mode is None else mode
    cbs, widths = fonttools_instance(font_bytes, location)
    upem = TTFont(io.BytesIO(font_bytes), lazy=True)["head"].unitsPerEm
    scale = 24.0 / upem
    blocks = {}
    for cp in sorted(cbs):
        if cp > 0xFFFF:
            continue
        adv_units = int(math.floor(widths[cp] + 0.5))
        adv_units = adv_units if 0 <= adv_units <= 65535 else 0
        adv_f = float(adv_units) * scale * 0.95
        adv = int(math.floor(adv_f + 0.5))
        info = oracle.GlyphInfo()
        info.id, info.advance = cp, adv
        bm = None
        rings = oracle.build_rings([(t[0],) + tuple(t[1:]) for t in cbs[cp]])
        if rings:
            dx = (adv - adv_f) / 2.0
            segs, pts = [], []
            for r in rings:
                p = r * scale
                p[:, 0] += dx
                p[:, 1] += 0.0
                pts.append(p)
                segs.append(np.concatenate([p[:-1], p[1:]], axis=1))
            allp = np.concatenate(pts)
            minx, miny, maxx, maxy = allp[:, 0].min(), allp[:, 1].min(), allp[:, 0].max(), allp[:, 1].max()
            if not (maxx <= minx and maxy <= miny):
                x0, y0 = int(math.floor(minx)) - 3, int(math.floor(miny)) - 3
                x1, y1 = int(math.ceil(maxx)) + 3, int(math.ceil(maxy)) + 3
                info.has_bitmap, info.x0, info.y0, info.w, info.h = 1, x0, y0, x1 - x0, y1 - y0
                info.width, info.height, info.left, info.top = info.w - 6, info.h - 6, x0 + 3, y1 - 24 - 3
                bm = oracle.sdf_render(np.concatenate(segs), x0, y0, x1 - x0, y1 - y0, mode)
        blocks.setdefault(cp // 256, []).append((info, bm))
    return {f"{name}/{b * 256}-{b * 256 + 255}.pbf": oracle.pbf_encode(name, b * 256, blocks.get(b, [])) for b in range(256)}
