"""Fixtures, hand-written faces and a strict restatement for the tests of rule G7 of csrc/host/ttf_face.hpp: the advances of a
placed `glyf` face without `HVAR`, from the deltas of gvar's phantom points n and n + 1.  No tests here.

The fixtures are the three variable Fira faces of tests/gvar_instances_kit.py with their `HVAR` deleted through fontTools.  The
hand-written faces use that kit's table writers, with `hmtx` advances that differ per glyph id, and put the phantom points on the
edges of the rule.  `restate` is written from the rule's text in numpy float32 / Python integers, not from the C++.  The
independent yardstick is fontTools: the width of a glyph of the glyph set at a location, read after it was drawn.
"""
import io
import struct

import numpy as np

import gvar_instances_kit as G
import variable_instances_kit as V

f32 = np.float32
ONE, HALF = G.ONE, G.HALF
NONE, DELTA, MALFORMED = 0, 1, 2
POSITIONS = ([0], [16384], [8192], [-8192], [5000])
_CACHE = {}


def without_hvar(kind="shear"):
    """gvar_instances_kit.variable_glyf_fira(kind) without its HVAR table: 315 glyphs whose gvar data carries phantom deltas"""
    key = ("nohvar", kind)
    if key not in _CACHE:
        from fontTools.ttLib import TTFont
        f = TTFont(io.BytesIO(G.variable_glyf_fira(kind)))
        del f["HVAR"]
        out = io.BytesIO()
        f.save(out)
        _CACHE[key] = out.getvalue()
        assert not V._table(_CACHE[key], "HVAR")
    return _CACHE[key]


# ---- the restatement of G7 -----------------------------------------------------------------------------------------------------

def point_count(t, gid):
    """n of glyph id gid's own entry (t: gvar_instances_kit._Tables); Malformed: the count cannot be read"""
    g = t.glyph(gid)
    if g is None:
        return 0
    if len(g) < 2:
        raise G.Malformed
    nc = G._i16(g, 0)
    if nc == 0:
        return 0
    if len(g) < 10:
        raise G.Malformed
    body = g[10:]
    if nc > 0:
        ends = [G._u16(body, 2 * k) for k in range(nc)]
        if ends[-1] == 0xFFFF:
            raise G.Malformed
        return ends[-1] + 1
    return len(G.components(body))


def phantom_sums(gvar, gid, coords, n):
    """(state, l, r): G1 to G4 for the tuples, the x deltas of points n and n + 1 of the applied ones"""
    l, r = f32(0), f32(0)
    n_axes, n_shared, shared_at, n_glyphs, flags, data_at = struct.unpack(">HHIHHI", gvar[4:20])
    if gid >= n_glyphs:
        return NONE, l, r
    if flags & 1:
        a, b = struct.unpack(">II", gvar[20 + 4 * gid:28 + 4 * gid])
    else:
        a, b = (2 * v for v in struct.unpack(">HH", gvar[20 + 2 * gid:24 + 2 * gid]))
    if a == b:
        return NONE, l, r
    if a > b or data_at + b > len(gvar):
        raise G.Malformed
    d = gvar[data_at + a:data_at + b]
    count, cursor = G._u16(d, 0), G._u16(d, 2)
    if count & 0x0FFF == 0:
        return NONE, l, r
    if cursor > len(d):
        raise G.Malformed
    shared_numbers = None
    if count & 0x8000:
        shared_numbers, cursor = G.read_points(d, cursor)
    h = 4
    for _ in range(count & 0x0FFF):
        size, index = G._u16(d, h), G._u16(d, h + 2)
        h += 4
        if index & 0x8000:
            peak = [G._i16(d, h + 2 * i) for i in range(n_axes)]
            h += 2 * n_axes
        else:
            if (index & 0x0FFF) >= n_shared:
                raise G.Malformed
            at = shared_at + (index & 0x0FFF) * 2 * n_axes
            peak = [G._i16(gvar, at + 2 * i) for i in range(n_axes)]
        start, end = [min(p, 0) for p in peak], [max(p, 0) for p in peak]
        if index & 0x4000:
            start = [G._i16(d, h + 2 * i) for i in range(n_axes)]
            end = [G._i16(d, h + 2 * n_axes + 2 * i) for i in range(n_axes)]
            h += 4 * n_axes
        if cursor + size > len(d):
            raise G.Malformed
        data = d[cursor:cursor + size]
        cursor += size
        scalar = f32(1)
        for i in range(n_axes):
            fac = V.axis_factor(coords[i], start[i], peak[i], end[i])
            scalar = f32(0) if fac == 0 or scalar == 0 else f32(scalar * fac)
        if scalar == 0:
            continue
        numbers, p = shared_numbers, 0
        if index & 0x2000:
            numbers, p = G.read_points(data, p)
        if numbers is None:
            values = G.read_deltas(data, p, 2 * (n + 4))            # all of them: x, then y
            l = f32(l + f32(f32(values[n]) * scalar))
            r = f32(r + f32(f32(values[n + 1]) * scalar))
            continue
        values = G.read_deltas(data, p, 2 * len(numbers))
        for k, number in enumerate(numbers):
            if number == n:
                l = f32(l + f32(f32(values[k]) * scalar))
            elif number == n + 1:
                r = f32(r + f32(f32(values[k]) * scalar))
    return DELTA, l, r


def restate_deltas(font_bytes, coords, n_ids=None):
    """(d float32[n], state uint8[n]) of every glyph id (n_ids: that many ids, those past numGlyphs included)"""
    t = G._Tables(font_bytes)
    n_ids = t.n_glyphs if n_ids is None else n_ids
    d, state = np.zeros(n_ids, np.float32), np.zeros(n_ids, np.uint8)
    for gid in range(n_ids):
        try:
            st, l, r = phantom_sums(t.gvar, gid, list(coords), point_count(t, gid))
        except G.Malformed:
            st, l, r = MALFORMED, f32(0), f32(0)
        state[gid] = st
        if st == DELTA:
            d[gid] = f32(r - l)
    return d, state


def hmtx_advances(font_bytes):
    hmtx, n_long = V._table(font_bytes, "hmtx"), struct.unpack(">H", V._table(font_bytes, "hhea")[34:36])[0]
    n = struct.unpack(">H", V._table(font_bytes, "maxp")[4:6])[0]
    return np.array([struct.unpack(">H", hmtx[4 * min(g, n_long - 1):4 * min(g, n_long - 1) + 2])[0] for g in range(n)], np.uint16)


def restate_advances(font_bytes, coords):
    """every glyph id's advance by G7, 0 for none (what Face::hor_advances gives)"""
    d, state = restate_deltas(font_bytes, coords)
    out = hmtx_advances(font_bytes)
    for g in range(len(out)):
        a = f32(out[g])
        if state[g] != MALFORMED:
            a = f32(a + f32(d[g] + f32(0.5)))
        whole = int(a)                                               # truncated
        out[g] = whole if 0 <= whole <= 65535 and a > -1 else 0
    return out


def fonttools_advances(font_bytes, location):
    """floor(width + 0.5) of every glyph id from fontTools' glyph set at the user-space location, the width read after draw"""
    import math
    return [int(math.floor(w + 0.5)) for w in fonttools_widths(font_bytes, location)]


def fonttools_widths(font_bytes, location):
    from fontTools.pens.basePen import NullPen
    from fontTools.ttLib import TTFont
    f = TTFont(io.BytesIO(font_bytes))
    location = {a.axisTag: location.get(a.axisTag, a.defaultValue) for a in f["fvar"].axes}
    gs = f.getGlyphSet(location=location)
    out = []
    for name in f.getGlyphOrder():
        g = gs[name]
        g.draw(NullPen())
        out.append(g.width)
    return out


def yardstick_files(font_bytes, location, name, oracle, mode=None):
    """gvar_instances_kit.yardstick_files with the widths fontTools has AFTER a glyph was drawn: without HVAR a glyph of the glyph
    set takes its width from the phantom points only while it is drawn, and that kit reads the width of a fresh glyph object
    (hmtx's).  Its callbacks are used as they are; only the widths it hands to its own arithmetic are replaced, for the call"""
    from fontTools.ttLib import TTFont
    cmap = TTFont(io.BytesIO(font_bytes)).getBestCmap()
    order = TTFont(io.BytesIO(font_bytes)).getGlyphOrder()
    drawn = dict(zip(order, fonttools_widths(font_bytes, location)))
    inner = G.fonttools_callbacks

    def callbacks(*a, **kw):
        cbs, widths, seen = inner(*a, **kw)
        return cbs, {cp: drawn[cmap[cp]] for cp in widths}, seen

    G.fonttools_callbacks = callbacks
    try:
        return G.yardstick_files(font_bytes, location, name, oracle, mode=mode)
    finally:
        G.fonttools_callbacks = inner


# ---- faces at the edges of G7 ----------------------------------------------------------------------------------------------------

def raw_deltas(runs):
    """G3 by hand: runs of ("z", count) | ("b", values) | ("w", values), each of 1 .. 64 values"""
    out = b""
    for kind, v in runs:
        if kind == "z":
            out += bytes([0x80 | (v - 1)])
        elif kind == "w":
            out += bytes([0x40 | (len(v) - 1)]) + b"".join(struct.pack(">h", x) for x in v)
        else:
            out += bytes([len(v) - 1]) + b"".join(struct.pack(">b", x) for x in v)
    return out


def _all_points_raw(runs, peak=(ONE,)):
    """a tuple over all points (private) whose deltas are the runs as given"""
    return G.tuple_of([], [], peak=list(peak), points=None, raw=b"\0" + raw_deltas(runs))


def _run_ending_at(kind, end, n_values=128):
    """128 values (64 points, x then y) where a run of `kind` covers values 50 .. end, byte runs the rest"""
    ramp = [((7 * i * i) % 97) - 40 for i in range(n_values)]
    mid = ramp[50:end + 1]
    runs = [("b", ramp[:50]), {"z": ("z", len(mid)), "b": ("b", mid), "w": ("w", [300 * v for v in mid])}[kind]]
    rest = ramp[end + 1:]
    for at in range(0, len(rest), 64):
        runs.append(("b", rest[at:at + 64]))
    return runs


SQUARE = [(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]


def _advances(n):
    return {i: 500 + 13 * i for i in range(n)}


def faces():
    """{case: (font bytes, glyph ids malformed at position [16384])}: one axis; hmtx advance of glyph id i: 500 + 13 i unless the
    case says otherwise"""
    if "faces" in _CACHE:
        return _CACHE["faces"]
    T, GV = G.tuple_of, G.glyph_variations
    sq, p60, empty = G.simple_entry([SQUARE]), G.simple_entry([G._polygon(60)]), b""
    plain = GV([T([1, -2, 3, -4, 6, 20, 0, 0], [5, 6, -7, 8, 0, 0, 9, 9], peak=[ONE], points=None)])    # l = 6, r = 20
    out = {}

    def add(case, entries, datas, malformed=(), advances=None, **gv):
        adv = _advances(len(entries))
        adv.update(advances or {})
        out[case] = (G.raw_font(entries, G.gvar_table(datas, **gv), advances=adv), set(malformed))

    # an empty entry (a loca range of length 0) has n = 0 and still its phantom points
    add("empty_entries", [sq, empty, empty, empty, empty],
        [plain, GV([T([10, 50, 0, 0], [0, 0, 7, 7], peak=[ONE], points=None)]),                         # exactly 4 deltas per axis
         GV([T([33], [4], peak=[ONE], points=[1])]),                                                   # a private list naming only 1
         GV([T([-9, 2], [1, 1], peak=[ONE], points=[0, 3])]),                                          # the left point alone
         b""])
    # a simple glyph of 60 points: lists naming n, n + 1, both, neither, numbers past n + 3, the two-byte count, shared numbers
    sub = lambda numbers, dx, **pack: GV([T(dx, [3] * len(numbers), peak=[ONE], points=numbers, **pack)])  # noqa: E731
    add("point_lists", [sq] + [p60] * 9,
        [plain, sub([60], [40]), sub([61], [-25]), sub([60, 61], [11, 70]), sub([0, 5, 62, 63], [9, 9, 9, 9]),
         sub([59, 60, 61, 64, 70, 40000], [1, 2, 30, 4, 5, 6]), sub([60, 61], [-8, 8], two_byte=True),
         sub([2, 61, 300, 600], [5, 77, 1, 1], words=True),
         GV([T([4, 14, 24], [1, 1, 1], shared=0, points="shared"), T([100, 200, 300], [0, 0, 0], peak=[HALF], inter=([0], [ONE]), points="shared")],
            shared_points=[3, 60, 61]),
         GV([T(G._ramp(64), G._ramp(64, 5), peak=[ONE], points=None)])], shared_tuples=[[ONE]])
    # G3: a zero, a byte and a word run each ending at x delta n - 1, n and n + 1; a run that spans the x / y boundary
    runs = [GV([_all_points_raw(_run_ending_at(kind, end))]) for kind in "zbw" for end in (59, 60, 61)]
    ramp = [((5 * i * i) % 61) - 30 for i in range(128)]
    span = GV([_all_points_raw([("b", ramp[:60]), ("w", [200 * v for v in ramp[60:68]]), ("b", ramp[68:128])])])
    zspan = GV([_all_points_raw([("b", ramp[:61]), ("z", 10), ("b", ramp[71:128])])])
    add("delta_runs", [sq] + [p60] * 11, [plain] + runs + [span, zspan])
    # an intermediate tuple whose scalar is 0 at every position of POSITIONS holds rubbish and is skipped; two tuples that both
    # move r (the order of the f32 sums); a left phantom delta
    skipped = T([], [], peak=[200], inter=([100], [300]), points=None, raw=b"\xff\xff\xff")
    add("scalars", [sq, p60, p60, sq],
        [plain, GV([T([60], [0], peak=[ONE], points=[61]), skipped, T([7], [0], peak=[-ONE], points=[61])]),
         GV([T([333], [1], peak=[ONE], points=[61]), T([-77], [1], peak=[HALF], inter=([0], [ONE]), points=[61]),
             T([1001], [1], peak=[ONE], points=[61])]),
         GV([T([0, 0, 0, 0, -31, 0, 0, 0], [0] * 8, peak=[ONE], points=None), T([0, 0, 0, 0, 17, 5, 0, 0], [0] * 8, peak=[-ONE], points=None)])])
    # composites: three records (n = 3); a composite whose component has phantom deltas of its own, which are not the composite's
    comp3 = G.composite_entry([(1, 100, 50, None), (1, -200, 0, (0.5, 0.25, -0.25, 0.75)), (2, 30, 30, None)])
    comp1 = G.composite_entry([(1, 0, 0, None)])
    add("composites", [sq, sq, p60, comp3, comp3, comp1, comp1],
        [plain, GV([T([0, 0, 0, 0, -50, 150, 0, 0], [0] * 8, peak=[ONE], points=None)]), sub([60, 61], [5, 6]),
         GV([T([24, -36, 12, 8, 88, 0, 0], [12, 60, 0, 0, 0, 0, 0], peak=[ONE], points=None)]), GV([T([40, -3], [0, 0], peak=[ONE], points=[2, 4])]),
         GV([T([9, 0, 21, 0, 0], [0] * 5, peak=[ONE], points=None)]), b""])
    # advances pushed out of 0 .. 65535 give none; the edges stay
    push = lambda v: GV([T([v], [0], peak=[ONE], points=[5])])  # noqa: E731
    add("out_of_range", [sq] * 7, [plain, push(-300), push(1000), push(-10), push(-12), push(535), push(536)],
        advances={1: 100, 2: 65000, 3: 10, 4: 10, 5: 65000, 6: 65000})
    # malformed: x deltas complete but y truncated; numbers that do not ascend; a tuple that ends inside its header
    y_cut = GV([G.tuple_of([], [], peak=[ONE], points=None, raw=b"\0" + raw_deltas([("b", [1, 2, 3, 4, 10, 90, 0, 0]), ("b", [1, 2, 3, 4, 5])]))])
    in_header = struct.pack(">HHHHh", 2, 10, 0, 0x8000, -ONE) + b"\0\0"                      # the second header has 2 of its 4 bytes
    add("malformed", [sq] * 6,
        [plain, y_cut, GV([T([1, 2], [3, 4], peak=[ONE], points=[5, 4])]), in_header,
         GV([T([1], [3], peak=[ONE], points="shared")], shared_points=[5, 5]), GV([T([21], [3], peak=[ONE], points=[5])])],
        malformed=(1, 2, 3, 4))
    _CACHE["faces"] = out
    return out


def truncated_face():
    """glyph id k owns the first k bytes of one glyph's data (two tuples, shared numbers naming the phantom points)"""
    if "cuts" not in _CACHE:
        full = G.glyph_variations([G.tuple_of([300, -2, 3], [5, 6, -700], peak=[HALF], inter=([100], [ONE]), points=[0, 4, 5]),
                                   G.tuple_of([1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1], shared=0)], shared_points=None)
        cuts = [full[:k] for k in range(len(full) + 1)]
        sq = G.simple_entry([SQUARE])
        _CACHE["cuts"] = G.raw_font([sq] * len(cuts), G.gvar_table(cuts, shared_tuples=[[ONE]]), advances=_advances(len(cuts)))
    return _CACHE["cuts"]


def padded_face(n_ids, at):
    """n_ids glyph ids, all empty entries without data but glyph id `at`: 60 points, a list naming n and n + 1"""
    key = ("pad", n_ids, at)
    if key not in _CACHE:
        entries, datas = [b""] * n_ids, [b""] * n_ids
        entries[at] = G.simple_entry([G._polygon(60)])
        datas[at] = G.glyph_variations([G.tuple_of([11, 70 + at], [3, 3], peak=[ONE], points=[60, 61])])
        _CACHE[key] = G.raw_font(entries, G.gvar_table(datas), advances=_advances(n_ids))
    return _CACHE[key]


def over_budget_face():
    """glyph id 1: an entry of 65535 points by its end point alone and 17 tuples of no data, all skipped at [16384]: tuples x
    (points + 4) passes VGSDF_GVAR_MAX_DELTAS = 2^20 in a few bytes"""
    if "budget" not in _CACHE:
        big = struct.pack(">hhhhhH", 1, 0, 0, 0, 0, 65534) + b"\0\0"
        heads = [(0x8000, struct.pack(">h", -ONE), b"")] * 17
        sq = G.simple_entry([SQUARE])
        plain = G.glyph_variations([G.tuple_of([1, -2, 3, -4, 6, 20, 0, 0], [0] * 8, peak=[ONE], points=None)])
        _CACHE["budget"] = G.raw_font([sq, big], G.gvar_table([plain, G.glyph_variations(heads)]), advances=_advances(2))
    return _CACHE["budget"]
