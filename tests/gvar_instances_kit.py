"""Fixtures, hand-written tables and a strict restatement for the tests of variable `glyf` faces (a glyf + gvar file rendered at
a chosen position of its design space).  No tests here.

The fixtures are built with fontTools from Fira Sans' glyf outlines (simple glyphs and composites), with masters whose advances
differ as in tests/variable_instances_kit.py, so that `HVAR` matters.  The hand-written faces put `gvar` / `glyf` / `loca` bytes
on the edges of the rules.  `restate` is written from the rules G1 to G6 as csrc/host/ttf_face.hpp states them, and from the
static walk's rules as the same file and tests/test_glyf_parts_host.py state them, in numpy float32 / Python integers, and not
from the C++.  `yardstick_files` builds the PBF files of an instance without the product's reader: the points and component
offsets fontTools has at the location, the callbacks of the static walk's rules over them in f64, the reference's arithmetic, the
oracle's ring builder, raster and encoder.
"""
import io
import struct

import numpy as np

from conftest import FIRA
import variable_instances_kit as V

f32 = np.float32
M, L, Q, C, Z = 0, 1, 2, 3, 4
SHEAR = (1.25, 0, 0.1, 1.05, 7, -3)      # (a): every point keeps an explicit delta
SCALE = (1.25, 0, 0, 1.05, 7, -3)        # (b): most tuples leave points to inference
EXACT_ONE_AXIS = [{"wght": 525}, {"wght": 650}, {"wght": 900}]
EXACT_TWO_AXES = [{"wght": 650, "wdth": 100}, {"wght": 775, "wdth": 150}, {"wght": 900, "wdth": 200}]

_CACHE = {}


def variable_glyf_fira(kind="shear"):
    """Fira Sans' first 700 glyph names, those kept whose components are among them (315 glyphs, simple and composite), as a
    glyf + gvar font with fvar and HVAR.  kind: "shear" (a), "scale" (b): one axis wght 400 .. 900 with a second master under
    SHEAR / SCALE whose composites have their offsets shifted; "two_axes" (c): wght with a master at 650 as well, and wdth
    100 .. 200 — tuples with intermediate regions, shared tuples."""
    if kind in _CACHE:
        return _CACHE[kind]
    from fontTools import varLib
    from fontTools.designspaceLib import AxisDescriptor, DesignSpaceDocument, SourceDescriptor
    from fontTools.fontBuilder import FontBuilder
    from fontTools.pens.transformPen import TransformPen
    from fontTools.pens.ttGlyphPen import TTGlyphPen
    from fontTools.ttLib import TTFont
    src = TTFont(FIRA)
    gs, glyf = src.getGlyphSet(), src["glyf"]
    first = src.getGlyphOrder()[:700]
    among = set(first)
    order = [g for g in first if not glyf[g].isComposite() or all(c.glyphName in among for c in glyf[g].components)]
    cmap = {cp: g for cp, g in src.getBestCmap().items() if g in order}

    def master(xform, style, width_of, shift):
        fb = FontBuilder(src["head"].unitsPerEm, isTTF=True)
        fb.setupGlyphOrder(order)
        fb.setupCharacterMap(cmap)
        glyphs = {}
        for g in order:
            pen = TTGlyphPen({n: None for n in order})
            if glyf[g].isComposite():
                for c in glyf[g].components:
                    t = (1, 0, 0, 1)
                    if hasattr(c, "transform"):
                        t = (c.transform[0][0], c.transform[0][1], c.transform[1][0], c.transform[1][1])
                    pen.addComponent(c.glyphName, t + (c.x + shift[0], c.y + shift[1]))
            else:
                gs[g].draw(TransformPen(pen, xform))
            glyphs[g] = pen.glyph()
        fb.setupGlyf(glyphs)
        # (left side bearing = xMin, as font tools write it: fontTools places a glyf outline by it, the crate does not look at it)
        fb.setupHorizontalMetrics({g: (width_of(i, gs[g].width), getattr(fb.font["glyf"][g], "xMin", 0)) for i, g in enumerate(order)})
        fb.setupHorizontalHeader(ascent=935, descent=-265)
        fb.setupNameTable({"familyName": "Synth Gvar", "styleName": style})
        fb.setupOS2()
        fb.setupPost()
        buf = io.BytesIO()
        fb.save(buf)
        return TTFont(io.BytesIO(buf.getvalue()))

    ds = DesignSpaceDocument()
    a = AxisDescriptor()
    a.tag, a.name, a.minimum, a.default, a.maximum = "wght", "Weight", 400, 400, 900
    ds.addAxis(a)
    second = SCALE if kind == "scale" else SHEAR
    masters = [(master((1, 0, 0, 1, 0, 0), "Regular", lambda i, w: w, (0, 0)), {"Weight": 400}),
               (master(second, "Bold", lambda i, w: int(w * 1.25) + 4 * (i % 3), (12, 0)), {"Weight": 900})]
    if kind == "two_axes":
        a = AxisDescriptor()
        a.tag, a.name, a.minimum, a.default, a.maximum = "wdth", "Width", 100, 100, 200
        ds.addAxis(a)
        for _, loc in masters:
            loc["Width"] = 100
        masters += [(master((1.125, 0, 0.25, 1, 2, 0), "Medium", lambda i, w: int(w * 1.125) + 2 * (i % 2), (4, 8)), {"Weight": 650, "Width": 100}),
                    (master((1.5, 0, -0.125, 1, 4, 0), "Wide", lambda i, w: int(w * 1.5) + 2 * (i % 5), (20, 0)), {"Weight": 400, "Width": 200}),
                    (master((1.75, 0, 0.25, 1.125, 0, 6), "Wide Bold", lambda i, w: int(w * 1.75) + 4 * (i % 3), (32, 4)), {"Weight": 900, "Width": 200})]
    for font, loc in masters:
        s = SourceDescriptor()
        s.font, s.location, s.familyName, s.styleName = font, loc, "Synth Gvar", "x"
        ds.addSource(s)
    vf, _, _ = varLib.build(ds, optimize=True)
    buf = io.BytesIO()
    vf.save(buf)
    _CACHE[kind] = buf.getvalue()
    return _CACHE[kind]


# ---- tables by hand ----------------------------------------------------------------------------------------------------------

def simple_entry(contours):
    """contours: lists of (x, y, on_curve) -> a `glyf` entry with word coordinates and one flag byte per point"""
    pts = [p for c in contours for p in c]
    ends, n = [], 0
    for c in contours:
        n += len(c)
        ends.append(n - 1)
    xs = [p[0] for p in pts]
    ys = [p[1] for p in pts]
    dx = [xs[0]] + [b - a for a, b in zip(xs, xs[1:])]
    dy = [ys[0]] + [b - a for a, b in zip(ys, ys[1:])]
    e = struct.pack(">hhhhh", len(contours), 0, 0, 0, 0) + b"".join(struct.pack(">H", v) for v in ends) + b"\0\0"
    e += bytes(1 if p[2] else 0 for p in pts) + b"".join(struct.pack(">h", v) for v in dx) + b"".join(struct.pack(">h", v) for v in dy)
    return e + b"\0" * (-len(e) % 2)


def composite_entry(records):
    """records: (child glyph id, dx, dy, None | scale | (a, b, c, d)) with word arguments"""
    e = struct.pack(">hhhhh", -1, 0, 0, 0, 0)
    for k, (child, dx, dy, xf) in enumerate(records):
        flags = 0x0003 | (0x0020 if k + 1 < len(records) else 0)
        tail = b""
        if isinstance(xf, tuple):
            flags |= 0x0080
            tail = b"".join(struct.pack(">h", int(round(v * 16384))) for v in xf)
        elif xf is not None:
            flags |= 0x0008
            tail = struct.pack(">h", int(round(xf * 16384)))
        e += struct.pack(">HHhh", flags, child, dx, dy) + tail
    return e + b"\0" * (-len(e) % 2)


def pack_points(numbers, words=False, run=128, two_byte=None):
    """G2: None -> all points; else the count (two-byte form from 128 on, or when asked) and runs of at most `run` increments"""
    if numbers is None:
        return b"\0"
    n = len(numbers)
    out = struct.pack(">H", 0x8000 | n) if (n >= 128 if two_byte is None else two_byte) else bytes([n])
    steps = [(b - a) & 0xFFFF for a, b in zip([0] + list(numbers), numbers)]
    for at in range(0, n, run):
        part = steps[at:at + run]
        w = words or any(s > 255 for s in part)
        out += bytes([(0x80 if w else 0) | (len(part) - 1)]) + b"".join(struct.pack(">H" if w else ">B", s) for s in part)
    return out


def pack_deltas(values, run=64, words=False):
    """G3: runs of at most `run` values: zero runs, byte runs, word runs as the values need (words=True: word runs only)"""
    out, at = b"", 0
    while at < len(values):
        part = values[at:at + run]
        kind = "z" if part[0] == 0 and not words else ("w" if words or not -128 <= part[0] <= 127 else "b")
        k = 0
        while k < len(part) and (("z" if part[k] == 0 and not words else ("w" if words or not -128 <= part[k] <= 127 else "b")) == kind):
            k += 1
        part = part[:k]
        if kind == "z":
            out += bytes([0x80 | (k - 1)])
        elif kind == "w":
            out += bytes([0x40 | (k - 1)]) + b"".join(struct.pack(">h", v) for v in part)
        else:
            out += bytes([k - 1]) + b"".join(struct.pack(">b", v) for v in part)
        at += k
    return out


def tuple_of(dx, dy, peak=None, shared=0, inter=None, points="shared", raw=None, **pack):
    """one tuple: peak = embedded peak (F2Dot14 integers, one per axis) or None (shared tuple index `shared`); inter = (start,
    end); points: "shared", None (private: all points) or a list (private).  raw: the serialized data as given"""
    index = shared if peak is None else 0x8000
    head = b"" if peak is None else b"".join(struct.pack(">h", v) for v in peak)
    if inter is not None:
        index |= 0x4000
        head += b"".join(struct.pack(">h", v) for v in inter[0]) + b"".join(struct.pack(">h", v) for v in inter[1])
    data = b""
    if points != "shared":
        index |= 0x2000
        data = pack_points(points, **{k: v for k, v in pack.items() if k in ("words", "two_byte")}, **({"run": pack["point_run"]} if "point_run" in pack else {}))
    data += pack_deltas(list(dx) + list(dy), **{k[6:]: v for k, v in pack.items() if k.startswith("delta_")})
    if raw is not None:
        data = raw
    return index, head, data


def glyph_variations(tuples, shared_points="none", count_field=None, size_of=None, data_offset=None, **pack):
    """G1: a glyph's variation data; shared_points: "none", None (all) or a list"""
    heads, datas = b"", b""
    lead = b"" if shared_points == "none" else pack_points(shared_points, **pack)
    for k, (index, head, data) in enumerate(tuples):
        size = len(data) if size_of is None else size_of(k, len(data))
        heads += struct.pack(">HH", size, index) + head
        datas += data
    count = (len(tuples) | (0 if shared_points == "none" else 0x8000)) if count_field is None else count_field
    off = 4 + len(heads) if data_offset is None else data_offset
    out = struct.pack(">HH", count, off) + heads + lead + datas
    return out + b"\0" * (-len(out) % 2)


def gvar_table(glyphs, shared_tuples=(), n_axes=1, long_offsets=True, glyph_count=None, version=0x00010000, axis_count=None):
    """glyphs: per glyph id its variation data (b"": none)"""
    offs, data = [0], b""
    for g in glyphs:
        data += g
        offs.append(len(data))
    n = len(glyphs) if glyph_count is None else glyph_count
    array = b"".join(struct.pack(">I", o) if long_offsets else struct.pack(">H", o // 2) for o in offs)
    shared_at = 20 + len(array)
    shared = b"".join(struct.pack(">h", v) for t in shared_tuples for v in t)
    return struct.pack(">IHHIHHI", version, n_axes if axis_count is None else axis_count, len(shared_tuples), shared_at, n,
                       1 if long_offsets else 0, shared_at + len(shared)) + array + shared + data


def raw_font(entries, gvar, n_axes=1, advances=None, cut_gvar=None, bearings=None):
    """a TrueType font whose glyph i is the raw entry entries[i] (code point 0x100 + i, long loca) with an fvar of n_axes axes
    (-1 .. 0 .. 1 in user space: a user value is its normalised one) and `gvar` as given (None: no gvar table).  advances,
    bearings: {glyph id: hmtx advance / left side bearing} (600 / 0 where not given)"""
    from fontTools.fontBuilder import FontBuilder
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables._g_l_y_f import Glyph
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    order = [f"g{i}" for i in range(len(entries))]
    fb = FontBuilder(1000, isTTF=True)
    fb.setupGlyphOrder(order)
    fb.setupCharacterMap({0x100 + i: g for i, g in enumerate(order)})
    fb.setupGlyf({g: Glyph() for g in order})
    fb.setupHorizontalMetrics({g: ((advances or {}).get(i, 600), (bearings or {}).get(i, 0)) for i, g in enumerate(order)})
    fb.setupHorizontalHeader(ascent=935, descent=-265)
    fb.setupNameTable({"familyName": "Synth Edge", "styleName": "Regular"})
    fb.setupOS2()
    fb.setupPost()
    fb.setupFvar([(("wght", "wdth", "slnt", "opsz")[i], -1, 0, 1, f"Axis{i}") for i in range(n_axes)], [])
    buf = io.BytesIO()
    fb.save(buf)
    f = TTFont(io.BytesIO(buf.getvalue()), recalcBBoxes=False, recalcTimestamp=False)
    data, offs = b"", [0]
    for e in entries:
        data += e + b"\0" * (-len(e) % 4)
        offs.append(len(data))
    glyf, loca = DefaultTable("glyf"), DefaultTable("loca")
    glyf.data, loca.data = data or b"\0\0\0\0", b"".join(struct.pack(">I", o) for o in offs)
    f["head"].indexToLocFormat = 1
    f["glyf"], f["loca"] = glyf, loca
    if gvar is not None:
        t = DefaultTable("gvar")
        t.data = gvar if cut_gvar is None else gvar[:cut_gvar]
        f["gvar"] = t
    out = io.BytesIO()
    f.save(out)
    return out.getvalue()


# ---- the restatement ---------------------------------------------------------------------------------------------------------

class Malformed(Exception):
    pass


TRACE = None      # a callable(what, *details): told what the restatement meets (tests/gvar_fuzz_kit.py counts its features with it)


def _t(*what):
    if TRACE is not None:
        TRACE(*what)


def _u16(b, at):
    if at + 2 > len(b):
        raise Malformed
    return (b[at] << 8) | b[at + 1]


def _i16(b, at):
    v = _u16(b, at)
    return v - 65536 if v >= 32768 else v


def _u8(b, at):
    if at >= len(b):
        raise Malformed
    return b[at]


def read_points(b, p):
    """G2 -> (None for all points | the numbers, position behind them)"""
    count = _u8(b, p)
    p += 1
    if count == 0:
        _t("point_count", "all", 0)
        return None, p
    if count & 0x80:
        count = ((count & 0x7F) << 8) | _u8(b, p)
        p += 1
        _t("point_count", "two_bytes", count)
    else:
        _t("point_count", "one_byte", count)
    out, number = [], 0
    while len(out) < count:
        control = _u8(b, p)
        p += 1
        _t("point_run", "words" if control & 0x80 else "bytes", min((control & 0x7F) + 1, count - len(out)))
        for _ in range((control & 0x7F) + 1):
            if len(out) == count:
                break
            if control & 0x80:
                step, p = _u16(b, p), p + 2
            else:
                step, p = _u8(b, p), p + 1
            nxt = (number + step) & 0xFFFF
            if out and nxt <= number:
                raise Malformed
            number = nxt
            out.append(nxt)
    return out, p


def read_deltas(b, p, n):
    """G3: n values of the stream at b[p:]"""
    out = []
    while len(out) < n:
        control = _u8(b, p)
        p += 1
        _t("delta_run", "zero" if control & 0x80 else "words" if control & 0x40 else "bytes", min((control & 0x3F) + 1, n - len(out)))
        for _ in range((control & 0x3F) + 1):
            if len(out) == n:
                break
            if control & 0x80:
                out.append(0)
            elif control & 0x40:
                out.append(_i16(b, p))
                p += 2
            else:
                v = _u8(b, p)
                out.append(v - 256 if v >= 128 else v)
                p += 1
    return out


def infer(p, pa, pb, da, db):
    """G5, one coordinate of one untouched point"""
    if pa == pb:
        _t("infer", "equal_coordinates_equal_deltas" if da == db else "equal_coordinates_unequal_deltas")
        return da if da == db else f32(0)
    if p <= min(pa, pb):
        _t("infer", "at_the_low_end" if p == min(pa, pb) else "below_the_pair")
        return da if pa < pb else db
    if p >= max(pa, pb):
        _t("infer", "at_the_high_end" if p == max(pa, pb) else "above_the_pair")
        return da if pa > pb else db
    _t("infer", "between")
    d = f32(f32(p - pa) / f32(pb - pa))
    return f32(f32(f32(f32(1) - d) * da) + f32(d * db))


def accumulate(gvar, gid, coords, n, xs=None, ys=None, last=None):
    """G1 to G5: [(ax, ay)] of the n + 4 points of glyph id gid; xs / ys / last None: a composite (nothing inferred)"""
    acc = [[f32(0), f32(0)] for _ in range(n + 4)]
    n_axes, n_shared, shared_at, n_glyphs, flags, data_at = struct.unpack(">HHIHHI", gvar[4:20])
    if gid >= n_glyphs:
        return acc
    if flags & 1:
        a, b = struct.unpack(">II", gvar[20 + 4 * gid:28 + 4 * gid])
    else:
        a, b = (2 * v for v in struct.unpack(">HH", gvar[20 + 2 * gid:24 + 2 * gid]))
    if a == b:
        return acc
    if a > b or data_at + b > len(gvar):
        raise Malformed
    d = gvar[data_at + a:data_at + b]
    count, cursor = _u16(d, 0), _u16(d, 2)
    n_tuples = count & 0x0FFF
    if n_tuples == 0:
        return acc
    if cursor > len(d):
        raise Malformed
    shared_numbers = None
    if count & 0x8000:
        shared_numbers, cursor = read_points(d, cursor)
    h = 4
    for _ in range(n_tuples):
        size, index = _u16(d, h), _u16(d, h + 2)
        h += 4
        if index & 0x8000:
            peak = [_i16(d, h + 2 * i) for i in range(n_axes)]
            h += 2 * n_axes
        else:
            if (index & 0x0FFF) >= n_shared:
                raise Malformed
            at = shared_at + (index & 0x0FFF) * 2 * n_axes
            peak = [_i16(gvar, at + 2 * i) for i in range(n_axes)]
        start, end = [min(p, 0) for p in peak], [max(p, 0) for p in peak]
        if index & 0x4000:
            start = [_i16(d, h + 2 * i) for i in range(n_axes)]
            end = [_i16(d, h + 2 * n_axes + 2 * i) for i in range(n_axes)]
            h += 4 * n_axes
        if cursor + size > len(d):
            raise Malformed
        data = d[cursor:cursor + size]
        cursor += size
        scalar = f32(1)
        for i in range(n_axes):
            fac = V.axis_factor(coords[i], start[i], peak[i], end[i])
            scalar = f32(0) if fac == 0 or scalar == 0 else f32(scalar * fac)
        _t("tuple", "embedded_peak" if index & 0x8000 else "shared_peak", "intermediate" if index & 0x4000 else "plain",
           "private_points" if index & 0x2000 else "shared_points", "skipped" if scalar == 0 else "applied" if scalar == 1 else "scaled")
        if scalar == 0:
            continue
        numbers, p = shared_numbers, 0
        if index & 0x2000:
            numbers, p = read_points(data, p)
        if numbers is None:
            values = read_deltas(data, p, 2 * (n + 4))
            for i in range(n + 4):
                acc[i][0] = f32(acc[i][0] + f32(f32(values[i]) * scalar))
                acc[i][1] = f32(acc[i][1] + f32(f32(values[n + 4 + i]) * scalar))
            continue
        values = read_deltas(data, p, 2 * len(numbers))
        got = {}
        for k, number in enumerate(numbers):
            if number < n + 4:
                got[number] = [f32(f32(values[k]) * scalar), f32(f32(values[len(numbers) + k]) * scalar)]
        add = dict(got)
        _t("phantom", any(n <= number < n + 4 for number in numbers), any(number >= n + 4 for number in numbers))
        if last is not None:
            first = 0
            while first < n:
                stop = first
                while stop + 1 < n and not last[stop]:
                    stop += 1
                touched = [i for i in range(first, stop + 1) if i in got]
                _t("contour", len(touched), stop + 1 - first, first in got, stop in got)
                if touched:
                    for i in range(first, stop + 1):
                        if i in got:
                            continue
                        before = max((t for t in touched if t < i), default=touched[-1])
                        behind = min((t for t in touched if t > i), default=touched[0])
                        add[i] = [infer(xs[i], xs[before], xs[behind], got[before][0], got[behind][0]),
                                  infer(ys[i], ys[before], ys[behind], got[before][1], got[behind][1])]
                first = stop + 1
        for i, (vx, vy) in add.items():
            acc[i][0] = f32(acc[i][0] + vx)
            acc[i][1] = f32(acc[i][1] + vy)
    return acc


class _Tables:
    def __init__(self, font_bytes):
        t = V._table
        self.glyf, self.loca, self.gvar = t(font_bytes, "glyf"), t(font_bytes, "loca"), t(font_bytes, "gvar")
        self.long = struct.unpack(">h", t(font_bytes, "head")[50:52])[0] != 0
        self.n_glyphs = struct.unpack(">H", t(font_bytes, "maxp")[4:6])[0]
        self.entries = min(self.n_glyphs + 1, len(self.loca) // (4 if self.long else 2))

    def glyph(self, gid):
        if gid + 1 >= self.entries:
            return None
        if self.long:
            a, b = struct.unpack(">II", self.loca[4 * gid:4 * gid + 8])
        else:
            a, b = (2 * v for v in struct.unpack(">HH", self.loca[2 * gid:2 * gid + 4]))
        return None if a >= b or b > len(self.glyf) else self.glyf[a:b]


def simple_points(body, nc):
    """the static walk's reading of a simple glyph's body -> (xs, ys, on, last) as integers / booleans; None: a lone point"""
    ends = [_u16(body, 2 * k) for k in range(nc)]
    if ends[-1] == 0xFFFF:
        raise Malformed
    n = ends[-1] + 1
    if n == 1:
        return None
    cur = 2 * nc
    cur += 2 + _u16(body, cur)
    if cur > len(body):
        raise Malformed
    flags = []
    while len(flags) < n:
        fl = _u8(body, cur)
        cur += 1
        run = 1
        if fl & 8:
            run += _u8(body, cur)
            cur += 1
        if run > n - len(flags):
            raise Malformed
        flags += [fl] * run

    def deltas(at, short, same):
        out = []
        for fl in flags:
            if fl & short:
                out.append(_u8(body, at) if fl & same else -_u8(body, at))
                at += 1
            elif fl & same:
                out.append(0)
            else:
                out.append(_i16(body, at))
                at += 2
        return out, at

    dx, y_at = deltas(cur, 2, 0x10)
    dy, _ = deltas(y_at, 4, 0x20)
    xs, ys, x, y = [], [], 0, 0
    for a, b in zip(dx, dy):
        x, y = (x + a + 32768) % 65536 - 32768, (y + b + 32768) % 65536 - 32768
        xs.append(x)
        ys.append(y)
    last, first = [False] * n, 0
    for k in range(nc):     # the end-point iterator: an end point that does not ascend still takes one point
        length = ends[0] + 1 if k == 0 else (ends[k] - ends[k - 1] if ends[k] > ends[k - 1] else 1)
        first += length
        if first - 1 < n:
            last[first - 1] = True
    for i in range(first, n):
        last[i] = True
    return xs, ys, [bool(fl & 1) for fl in flags], last


def emit(pts, on, last, tr, num, out):
    """the static walk's emitter over points (x, y) of number type num (f32, or float for the yardstick): out gets
    (kind, [coordinates]); tr = None or (a, b, c, d, e, f)"""
    half = num(0.5)

    def t(p):
        if tr is None:
            return [p[0], p[1]]
        a, b, c, d, e, f = tr
        return [num(num(num(a * p[0]) + num(c * p[1])) + e), num(num(num(b * p[0]) + num(d * p[1])) + f)]

    def mid(p, q):
        return (num(p[0] + num(half * num(q[0] - p[0]))), num(p[1] + num(half * num(q[1] - p[1]))))

    start = lead = pend = None
    for p, o, l in zip(pts, on, last):
        if start is None:
            if o:
                start = p
                out.append((M, t(p)))
            elif lead is not None:
                start, pend = mid(lead, p), p
                out.append((M, t(start)))
            else:
                lead = p
        elif pend is not None:
            cp = pend
            if o:
                pend = None
                out.append((Q, t(cp) + t(p)))
            else:
                pend = p
                out.append((Q, t(cp) + t(mid(cp, p))))
        elif o:
            out.append((L, t(p)))
        else:
            pend = p
        if l:
            if lead is not None and pend is not None:
                cp, pend = pend, None
                out.append((Q, t(cp) + t(mid(cp, lead))))
            if start is not None and lead is not None:
                out.append((Q, t(lead) + t(start)))
            elif start is not None and pend is not None:
                out.append((Q, t(pend) + t(start)))
            elif start is not None:
                out.append((L, t(start)))
            start = lead = pend = None
            out.append((Z, []))


def _then(p, k, num):
    a, b, c, d, e, f = p
    return (num(num(a * k[0]) + num(c * k[1])), num(num(b * k[0]) + num(d * k[1])), num(num(a * k[2]) + num(c * k[3])),
            num(num(b * k[2]) + num(d * k[3])), num(num(num(a * k[4]) + num(c * k[5])) + e), num(num(num(b * k[4]) + num(d * k[5])) + f))


def components(body):
    """the records the static walk reads of a composite's body: [(child, [a, b, c, d, e, f] as f32)]"""
    out, p = [], 0
    try:
        while True:
            flags, child = _u16(body, p), _u16(body, p + 2)
            p += 4
            k = [f32(1), f32(0), f32(0), f32(1), f32(0), f32(0)]
            if flags & 2:
                if flags & 1:
                    k[4], k[5], p = f32(_i16(body, p)), f32(_i16(body, p + 2)), p + 4
                else:
                    _u8(body, p + 1)
                    k[4], k[5], p = f32(_u8(body, p) - 256 * (body[p] >> 7)), f32(body[p + 1] - 256 * (body[p + 1] >> 7)), p + 2
            two = lambda at: f32(f32(_i16(body, at)) / f32(16384))  # noqa: E731
            if flags & 0x80:
                k[0], k[1], k[2], k[3], p = two(p), two(p + 2), two(p + 4), two(p + 6), p + 8
            elif flags & 0x40:
                k[0], k[3], p = two(p), two(p + 2), p + 4
            elif flags & 0x08:
                k[0] = k[3] = two(p)
                p += 2
            out.append((child, k))
            if not flags & 0x20:
                break
    except Malformed:
        pass
    return out


IDENTITY = (f32(1), f32(0), f32(0), f32(1), f32(0), f32(0))


def walk(t, coords, gid, depth, tr, out):
    """G5 / G6 over the tree of glyph id gid: False where the reader's outline_glyph returns false"""
    g = t.glyph(gid)
    if g is None:
        return depth != 0
    if depth >= 32 or len(g) < 2:
        return False
    nc = _i16(g, 0)
    body = g[10:]
    try:
        if nc > 0:
            if len(g) < 10:
                return False
            pts = simple_points(body, nc)
            if pts is None:
                return True
            xs, ys, on, last = pts
            _t("glyph", "simple", depth, sum(last), len(xs))
            acc = accumulate(t.gvar, gid, coords, len(xs), xs, ys, last)
            moved = [(f32(f32(x) + a[0]), f32(f32(y) + a[1])) for x, y, a in zip(xs, ys, acc)]
            emit(moved, on, last, None if all(a == b for a, b in zip(tr, IDENTITY)) else tr, f32, out)
            return True
        if nc == 0 or len(g) < 10:
            return nc == 0
        recs = components(body)
        _t("glyph", "composite", depth, len(recs), any(not all(a == b for a, b in zip(k[:4], IDENTITY[:4])) for _, k in recs))
        acc = accumulate(t.gvar, gid, coords, len(recs))
    except Malformed:
        return False
    for (child, k), a in zip(recs, acc):
        k[4], k[5] = f32(k[4] + a[0]), f32(k[5] + a[1])
        if not walk(t, coords, child, depth + 1, _then(tr, k, f32), out):
            return False
    return True


def restate(font_bytes, coords):
    """the command table of the face at coords: {cmd_off, dat_off, kinds, coords, ok: per glyph id what outline_glyph returns}"""
    t = _Tables(font_bytes)
    cmd_off, dat_off, kinds, floats, ok = [0], [0], [], [], []
    for gid in range(t.n_glyphs):
        out = []
        ok.append(walk(t, list(coords), gid, 0, IDENTITY, out))
        for kind, c in out:
            kinds.append(kind)
            floats += c
        cmd_off.append(len(kinds))
        dat_off.append(len(floats))
    return {"cmd_off": np.array(cmd_off, np.uint32), "dat_off": np.array(dat_off, np.uint32), "kinds": np.array(kinds, np.uint8),
            "coords": np.array(floats, np.float32), "ok": ok}


# ---- fontTools at a location, and the independent yardstick -----------------------------------------------------------------

def fonttools_callbacks(font_bytes, location, exact=True, normalized=False):
    """({cp: [(kind, x1, y1, x2, y2, x, y)]}, {cp: width}, every coordinate seen) from the points and component offsets of
    fontTools' glyph set at `location`, the static walk's emitter and transforms over them in f64.  exact: asserts that every
    coordinate and width is a multiple of 1/8 below 2^20 (the positions the yardstick is valid at: f32 and f64 then agree)"""
    from fontTools.pens.pointPen import AbstractPointPen
    from fontTools.ttLib import TTFont
    f = TTFont(io.BytesIO(font_bytes))
    if not normalized:
        location = {a.axisTag: location.get(a.axisTag, a.defaultValue) for a in f["fvar"].axes}
    gs, cmap = f.getGlyphSet(location=location, normalized=normalized), f.getBestCmap()
    seen = []

    class Pen(AbstractPointPen):
        def __init__(self):
            self.contours, self.comps = [], []

        def beginPath(self, **kw):
            self.contours.append([])

        def endPath(self):
            pass

        def addPoint(self, pt, segmentType=None, **kw):
            self.contours[-1].append((float(pt[0]), float(pt[1]), segmentType is not None))

        def addComponent(self, name, transform, **kw):
            self.comps.append((name, tuple(float(v) for v in transform)))

    def draw(name, tr, out, depth=0):
        pen = Pen()
        gs[name].drawPoints(pen)
        for c in pen.contours:
            if len(c) == 1 and len(pen.contours) == 1:
                continue
            seen.extend(v for p in c for v in p[:2])
            emit([(p[0], p[1]) for p in c], [p[2] for p in c], [False] * (len(c) - 1) + [True],
                 None if tr == (1.0, 0.0, 0.0, 1.0, 0.0, 0.0) else tr, float, out)
        for child, k in pen.comps:
            seen.extend(k[4:])
            draw(child, _then(tr, k, float), out, depth + 1)

    cbs, widths = {}, {}
    for cp, name in cmap.items():
        out = []
        draw(name, (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), out)
        cbs[cp] = [(kind,) + {M: lambda c: (0.0,) * 4 + tuple(c), L: lambda c: (0.0,) * 4 + tuple(c), Z: lambda c: (0.0,) * 6,
                              Q: lambda c: (c[0], c[1], 0.0, 0.0, c[2], c[3])}[kind](c) for kind, c in out]
        widths[cp] = gs[name].width
    if exact:
        for v in seen + list(widths.values()) + [v for c in cbs.values() for t in c for v in t[1:]]:
            assert v * 16 == int(v * 16) and abs(v) < 1 << 20, v
        for w in widths.values():
            assert w * 8 == int(w * 8), w
    return cbs, widths, seen


def yardstick_files(font_bytes, location, name, oracle, mode=None):
    """{path: bytes} of the instance at `location` under font id `name`, without the product: fonttools_callbacks' callbacks and
    widths, advance = floor(width + 0.5), the arithmetic of the reference's render_glyph in f64, the oracle's rings, raster and
    encoder (what variable_instances_kit.yardstick_files does with the callbacks of a CFF2 instance)"""
    import math
    from fontTools.ttLib import TTFont
    mode = oracle.PRECISE if mode is None else mode
    cbs, widths, _ = fonttools_callbacks(font_bytes, location)
    scale = 24.0 / TTFont(io.BytesIO(font_bytes), lazy=True)["head"].unitsPerEm
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


# ---- what the tests compare with ---------------------------------------------------------------------------------------------

CLOSE = 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def callbacks_of(o):
    """{code point: [(kind, x1, y1, x2, y2, x, y)]} of FontManager.record_outlines"""
    out = {}
    for i, cp in enumerate(o["ids"]):
        got = o["cmds"][o["cmd_off"][i]:o["cmd_off"][i + 1]]
        out[int(cp)] = [(int(c["kind"]),) + ((0.0,) * 6 if c["kind"] == CLOSE else tuple(float(c[k]) for k in ("x1", "y1", "x2", "y2", "x", "y")))
                        for c in got]
    return out


def same_family(got, want):
    for k in ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x"):
        assert bits(got[k]) == bits(want[k]), k


# ---- faces at the edges of G1 to G6 -------------------------------------------------------------------------------------------

EDGE_POSITIONS = ([16384], [8192], [-8192], [5000], [0])
ONE, HALF = 16384, 8192


def _polygon(n, on_every=1, at=(0, 0)):
    """n points on a rough circle, integer coordinates, every on_every-th on the curve"""
    import math
    return [(at[0] + int(500 + 400 * math.cos(2 * math.pi * i / n)), at[1] + int(500 + 400 * math.sin(2 * math.pi * i / n)), i % on_every == 0)
            for i in range(n)]


def _ramp(n, k=7, lo=-90):
    return [lo + (k * i) % 181 for i in range(n)]


def edge_faces():
    """{case: (font bytes, glyph ids whose data is malformed)}: one axis unless the case says otherwise; every glyph id's data is
    what the case is about, glyph id 0 a plain square with one all-points tuple"""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    square = [(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]
    sq = simple_entry([square])
    all8 = lambda k=1: tuple_of([k * v for v in (1, -2, 3, -4, 0, 0, 0, 0)], [k * v for v in (5, 6, -7, 8, 0, 0, 0, 0)], peak=[ONE], points=None)  # noqa: E731
    plain = glyph_variations([all8()])
    out = {}

    def add(case, entries, datas, malformed=(), **kw):
        gv = {k: kw.pop(k) for k in ("shared_tuples", "n_axes", "long_offsets", "glyph_count") if k in kw}
        out[case] = (raw_font(entries, gvar_table(datas, **gv), n_axes=gv.get("n_axes", 1)), set(malformed))

    # G1: 0, 1 and 3 tuples; an empty range; glyph ids past glyphCount; the short offset form
    three = glyph_variations([tuple_of([1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1], shared=0),
                              tuple_of([10, -20], [30, -40], peak=[HALF], inter=([0], [ONE]), points=[1, 3]),
                              tuple_of([-5] * 8, [300] * 8, shared=1, points=None)], shared_points=None)
    add("tuple_counts", [sq] * 5, [plain, glyph_variations([]), b"", three], shared_tuples=[[ONE], [-ONE]], glyph_count=4)
    add("short_offsets", [sq] * 3, [plain, b"", three], shared_tuples=[[ONE], [-ONE]], long_offsets=False)
    # G2: counts 127 / 128 (the two-byte form), 129 numbers in two runs, 8- and 16-bit runs, numbers at and past the count
    big = simple_entry([_polygon(100), _polygon(160, 2, (900, 0))])
    n_big = 260

    def subset(numbers, **pack):
        return glyph_variations([tuple_of(_ramp(len(numbers)), _ramp(len(numbers), 11), peak=[ONE], points=numbers, **pack)])

    add("point_numbers", [sq] + [big] * 9,
        [plain, subset(list(range(0, 254, 2))), subset(list(range(0, 256, 2))), subset(list(range(1, 259, 2)), point_run=100),
         subset(list(range(0, 127)), two_byte=True), subset([3, 9, 200, 259], words=True), subset([0, 5, 259, 260, 263, 264, 300, 40000]),
         glyph_variations([tuple_of(_ramp(40), _ramp(40, 3), shared=0, points="shared")], shared_points=list(range(90, 130))),
         glyph_variations([tuple_of([], [], peak=[ONE], points=[], two_byte=True)]),
         subset([0, 300, 600, 900, 1200], words=True)], shared_tuples=[[ONE]])
    add("point_numbers_that_descend", [sq] * 5,
        [plain, glyph_variations([tuple_of([1, 2], [3, 4], peak=[ONE], points=[2, 1])]),
         glyph_variations([tuple_of([1, 2], [3, 4], peak=[ONE], points=[2, 2])]),
         glyph_variations([tuple_of([1, 2], [3, 4], peak=[ONE], points=[3, 65538])]),              # 3, then a step of 65535: the u16 sum wraps to 2
         glyph_variations([tuple_of([1], [3], peak=[ONE], points="shared")], shared_points=[5, 4])], malformed=(1, 2, 3, 4))
    # G3: runs of 64 and of 65 values; zero, byte and word runs
    p60 = simple_entry([_polygon(60)])        # 64 points with the phantom ones
    p61 = simple_entry([_polygon(61)])        # 65
    zeros_then = lambda n: [0] * 20 + _ramp(n - 40) + [0] * 20  # noqa: E731
    add("delta_runs", [sq, p60, p61, p61, p61, p60],
        [plain, glyph_variations([tuple_of(_ramp(64), _ramp(64, 5), peak=[ONE], points=None)]),
         glyph_variations([tuple_of(_ramp(65), _ramp(65, 5), peak=[ONE], points=None)]),
         glyph_variations([tuple_of([300 * v for v in _ramp(65)], zeros_then(65), peak=[ONE], points=None)]),
         glyph_variations([tuple_of(_ramp(65), _ramp(65, 5), peak=[ONE], points=None, delta_words=True, delta_run=33)]),
         glyph_variations([tuple_of([0] * 64, [0] * 63 + [-32768], peak=[ONE], points=None)])])
    # G4: scalar 0, the negative side, embedded peaks, intermediate regions, shared indices (one past the count); two axes
    add("scalars", [sq] * 7,
        [plain, glyph_variations([tuple_of([9] * 8, [9] * 8, peak=[-ONE], points=None)]),
         glyph_variations([tuple_of([40] * 8, [-40] * 8, peak=[HALF], inter=([4096], [ONE]), points=None), all8(3)]),
         glyph_variations([tuple_of([7] * 8, [1] * 8, shared=1, points=None), tuple_of([100] * 8, [0] * 8, shared=0, points=None)]),
         glyph_variations([all8(), tuple_of([7] * 8, [1] * 8, shared=2, points=None)]),
         # a skipped tuple (scalar 0 on the positive side) whose data is rubbish, in front of a good one
         glyph_variations([tuple_of([], [], peak=[-ONE], points=None, raw=b"\xff\xff\xff"), all8(2)]),
         glyph_variations([tuple_of([1] * 8, [1] * 8, peak=[0], points=None)])],
        shared_tuples=[[ONE], [-HALF]], malformed=(4,))
    add("two_axes", [sq] * 3,
        [glyph_variations([tuple_of([16] * 8, [32] * 8, peak=[ONE, 0], points=None)]),
         glyph_variations([tuple_of([16] * 8, [32] * 8, peak=[ONE, ONE], points=None), tuple_of([-48] * 8, [80] * 8, shared=0, points=None),
                           tuple_of([5] * 8, [6] * 8, peak=[HALF, HALF], inter=([0, 0], [ONE, ONE]), points=None)]),
         glyph_variations([tuple_of([1000] * 8, [1000] * 8, peak=[0, -ONE], points=None)])], shared_tuples=[[0, ONE]], n_axes=2)
    # G5: inference
    c1 = [(0, 0, True), (100, 0, True), (200, 50, False), (300, 100, True), (300, 300, True), (150, 400, False), (0, 300, True), (-50, 150, True)]
    c2 = [(1000, 0, True), (1100, 0, True), (1100, 100, True)]
    c3 = [(2000, 0, True)]                                        # a one-point contour
    c4 = [(3000, 10, True), (3000, 10, False), (3100, 10, True), (3000, 90, True)]   # equal coordinates
    shape = simple_entry([c1, c2, c3, c4])                        # points 0-7, 8-10, 11, 12-15, phantom 16-19

    def touch(numbers, dx, dy):
        return glyph_variations([tuple_of(dx, dy, peak=[ONE], points=numbers)])

    add("inference", [sq] + [shape] * 10,
        [plain, touch([0], [10], [-20]),                                       # one touched point in its contour: all follow it
         touch([1, 6], [30, -10], [8, 40]),                                  # two: between, outside, and the wrap over the end
         touch([6, 7], [30, -10], [8, 40]),                                  # ... the pair at the contour's end
         touch([0, 3, 9], [5, 50, 7], [9, -9, 3]),                           # two contours touched, two not
         touch([11], [60], [60]),                                            # the one-point contour alone
         touch([12, 13], [7, 7], [20, -20]),                                 # equal coordinates: equal deltas in x, unequal in y
         touch([12, 13, 14], [7, 9, 11], [20, -20, 5]),
         touch([16, 19], [100, -100], [50, -50]),                            # phantom points only: nothing moves
         touch([2, 5, 10, 17], [33, -77, 12, 5], [-3, 90, -45, 5]),          # off-curve points touched
         glyph_variations([tuple_of([3, 5], [7, 9], shared=0, points=[4, 8]), tuple_of([50, -70, 20], [0, 10, 0], shared=0, points=[0, 4, 15]),
                           tuple_of(_ramp(20), _ramp(20, 3), peak=[-ONE], points=None)])], shared_tuples=[[ONE]])
    # G6: composites of one and two levels, a scaled parent in between; deltas of component points, of phantom points, past them
    comp1 = composite_entry([(1, 100, 50, None), (1, -200, 0, (0.5, 0.25, -0.25, 0.75))])
    comp2 = composite_entry([(3, 10, 20, 0.75), (2, 700, -100, None), (3, 0, 0, (1.5, 0, 0, -1.0))])
    lone = simple_entry([[(5, 5, True)]])
    comp3 = composite_entry([(6, 1, 1, None), (2, 30, 30, None)])              # a lone point and a simple glyph
    add("composites", [sq, shape, sq, comp1, comp2, comp2, lone, comp3],
        [plain, touch([1, 6], [30, -10], [8, 40]), glyph_variations([all8(4)]),
         glyph_variations([tuple_of([24, -36, 0, 0, 0, 0], [12, 60, 0, 0, 0, 0], peak=[ONE], points=None)]),
         glyph_variations([tuple_of([15, 25], [35, -45], peak=[ONE], points=[0, 2]), tuple_of([9], [9], peak=[HALF], inter=([0], [ONE]), points=[1])]),
         glyph_variations([tuple_of([15, 25, 1, 1], [35, -45, 1, 1], peak=[-ONE], points=[1, 2, 4, 9])]),
         touch([0], [10], [10]), glyph_variations([tuple_of([8, 8, 0, 0, 0, 0], [-8, 8, 0, 0, 0, 0], peak=[ONE], points=None)])])
    # a malformed child, a malformed composite: what was delivered before stays
    bad = glyph_variations([tuple_of([], [], peak=[ONE], points=None, raw=b"\x03\x01\x02")])
    add("composites_malformed", [sq, sq, composite_entry([(0, 0, 0, None), (1, 50, 50, None), (0, 900, 0, None)]), composite_entry([(0, 0, 0, None)])],
        [plain, bad, glyph_variations([all8()[:2] + (pack_deltas([1, 2, 3, 0, 0, 0, 0] + [0] * 7),)]), bad], malformed=(1, 2, 3))
    # truncation at every byte of a glyph's data (glyph id k owns the first k bytes), and of data with shared numbers
    full = glyph_variations([tuple_of([300, -2, 3], [5, 6, -700], peak=[HALF], inter=([100], [ONE]), points=[0, 2, 3]),
                             tuple_of([1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1], shared=0)], shared_points=None)
    cuts = [full[:k] for k in range(len(full) + 1)]
    out["truncated"] = (raw_font([sq] * len(cuts), gvar_table(cuts, shared_tuples=[[ONE]])), None)
    _CACHE["edge"] = out
    return out


def unreadable_gvars():
    """{case: font bytes} of faces parse_at refuses: no gvar, another version, another axis count, a header / shared tuples / an
    offset array that leave the table"""
    square = simple_entry([[(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]])
    datas = [glyph_variations([tuple_of([1] * 8, [1] * 8, peak=[ONE], points=None)])] * 2
    good = gvar_table(datas, shared_tuples=[[ONE]])
    array_end = 20 + 4 * 3
    return {"none": raw_font([square] * 2, None), "version": raw_font([square] * 2, gvar_table(datas, version=0x00020000)),
            "axis_count": raw_font([square] * 2, gvar_table(datas, axis_count=2)), "two_axes_file": raw_font([square] * 2, good, n_axes=2),
            "header": raw_font([square] * 2, good, cut_gvar=19), "offset_array": raw_font([square] * 2, good, cut_gvar=array_end - 1),
            "shared_tuples": raw_font([square] * 2, good, cut_gvar=array_end + 1)}
