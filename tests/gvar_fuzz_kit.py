"""A kit (no tests): seeded random glyf + gvar faces on top of tests/gvar_instances_kit.py, whose table writers, restatement of
rules G1 to G6 and fontTools reading it uses, and of tests/phantom_advances_kit.py for rule G7 (no face here has an `HVAR`).

face(seed, n) makes a face of 1, 2 or 3 axes (seed % 3): simple glyphs of 1 to 6 contours of 1 to 70 points, composites up to
three levels deep with and without transforms, and per glyph 0 to 8 tuples — shared and embedded peaks, intermediate regions,
private, shared and all-points lists in both count spellings with runs cut at 1, 127 and 128 in byte or word form, deltas in
zero, byte and word runs cut at 1, 63 and 64, touched sets that leave inference every case of its rule (none, one, all, a
contour's first or last point, equal coordinates under unequal deltas, targets outside the pair), phantom points touched or not.
Only well-formed data is written (the device refuses a face with one malformed glyph id), and a face is kept only if the
restatement runs every glyph id at every position of the face within MAX_WORK tuples x points.

features() says what a face reached at a position, from what the restatement itself met (gvar_instances_kit.TRACE), FEATURES what
a corpus must reach; tracked_restate() is the restatement over numbers that count their own f32 roundings; MUTANTS are
restatements with one rule broken each.
"""
import contextlib
import random

import numpy as np

import charstring_fuzz_kit as F
import gvar_instances_kit as G
import phantom_advances_kit as P
import variable_instances_kit as V

MAX_WORK = 4096
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
N_GLYPHS = 128
ONE = G.ONE


def _peak(rng, n_axes):
    p = [rng.choice((ONE, -ONE, ONE, 8192, -8192, 0, rng.randint(-ONE, ONE))) for _ in range(n_axes)]
    if not any(p):
        p[rng.randrange(n_axes)] = ONE
    return p


def _region(rng, peak):
    """an intermediate region around the peak; now and then one the rules take for "no region" (factor 1)"""
    start, end = [], []
    for p in peak:
        if rng.random() < 0.06:
            s, e = sorted((rng.randint(-ONE, 0), rng.randint(0, ONE)))          # start < 0 < end
        elif p > 0:
            s, e = rng.randint(0, p), rng.randint(p, ONE)
        elif p < 0:
            s, e = rng.randint(-ONE, p), rng.randint(p, 0)
        else:
            s = e = 0
        start.append(s)
        end.append(e)
    return start, end


def _deltas(rng, n):
    kind = rng.choice(("small", "small", "mixed", "wide", "zeros"))
    out = []
    while len(out) < n:
        run = rng.choice((1, 2, 5, 63, 64, 65, rng.randint(1, 30)))
        k = kind if kind != "mixed" else rng.choice(("small", "wide", "zeros"))
        out += [0 if k == "zeros" else rng.randint(-100, 100) if k == "small" else rng.randint(-3000, 3000) for _ in range(run)]
    return out[:n]


def _numbers(rng, contours, n):
    """a touched set (ascending point numbers): one of the cases of the inference rule, and the phantom points or not"""
    firsts, at = [], 0
    for c in contours:
        firsts.append((at, at + len(c) - 1))
        at += len(c)
    case = rng.choice(("one", "all", "first", "last", "ends", "some", "some", "sparse", "phantom_only", "past_only"))
    if n >= 128 and rng.random() < 0.6:
        case = rng.choice(("all", "most"))
    if case == "all":
        out = list(range(n))
    elif case == "one":
        out = [rng.randrange(n)]
    elif case == "first":
        out = sorted({a for a, _ in rng.sample(firsts, rng.randint(1, len(firsts)))})
    elif case == "last":
        out = sorted({b for _, b in rng.sample(firsts, rng.randint(1, len(firsts)))})
    elif case == "ends":
        out = sorted({v for pair in firsts for v in pair})
    elif case == "some":
        out = sorted(rng.sample(range(n), rng.randint(1, n)))
    elif case == "most":
        out = sorted(rng.sample(range(n), rng.randint(127, n)))
    elif case == "sparse":
        out = sorted(rng.sample(range(n), min(n, rng.randint(2, 4))))
    else:
        out = []
    if case == "phantom_only" or rng.random() < 0.4:
        out += sorted(rng.sample(range(n, n + 4), rng.randint(1, 4)))
    if case == "past_only" or rng.random() < 0.1:
        out += sorted(rng.sample(range(n + 4, n + 400), rng.randint(1, 3)))
    return out


def _pack(rng):
    pack = {"delta_run": rng.choice((1, 63, 64, 64, 64)), "delta_words": rng.random() < 0.15, "point_run": rng.choice((1, 127, 128, 128, 128)),
            "words": rng.random() < 0.3}
    if rng.random() < 0.3:
        pack["two_byte"] = True
    return pack


def _tuples(rng, n_axes, shared_peaks, contours, n):
    """-> (tuples, shared numbers or "none") for a glyph of n points (a composite: contours None, n records)"""
    count = rng.choice((0, 1, 1, 2, 2, 3, 4, rng.randint(5, 8)))
    shared = "none"
    if count and rng.random() < 0.4:
        shared = None if rng.random() < 0.3 else (_numbers(rng, contours, n) if contours else sorted(rng.sample(range(n + 4), rng.randint(1, n + 4))))
    out = []
    for _ in range(count):
        peak = None if rng.random() < 0.4 else _peak(rng, n_axes)
        index = rng.randrange(len(shared_peaks))
        inter = _region(rng, shared_peaks[index] if peak is None else peak) if rng.random() < 0.35 else None
        r = rng.random()
        if shared != "none" and r < 0.4:
            points, k = "shared", (n + 4 if shared is None else len(shared))
        elif r < 0.6:
            points, k = None, n + 4
        else:
            points = _numbers(rng, contours, n) if contours else sorted(rng.sample(range(n + 4), rng.randint(1, n + 4)))
            k = len(points)
        pack = _pack(rng)
        if isinstance(points, list) and len(points) >= 127:
            pack.update(words=rng.random() < 0.5, point_run=rng.choice((127, 128, 128)))
        dx, dy = _deltas(rng, k), _deltas(rng, k)
        if contours and isinstance(points, list) and rng.random() < 0.3:
            # two touched neighbours of equal coordinates get unequal deltas (the generator of the outlines makes such pairs)
            flat = [p for c in contours for p in c]
            for a, b in zip(points, points[1:]):
                if b < n and flat[a][0] == flat[b][0]:
                    dx[points.index(b)] = dx[points.index(a)] + rng.choice((-7, 9))
        out.append((dict(peak=peak, shared=index, inter=inter, points=points, **pack), dx, dy))
    return out, shared


def _contours(rng):
    out, big = [], rng.random() < 0.14                     # (big: enough points for runs of 127 and 128 numbers)
    for _ in range(3 if big else rng.choice((1, 1, 2, 2, 3, 4, 5, 6))):
        k = rng.randint(60, 70) if big else rng.choice((1, 2, 3, 4, 5, 8, 12, rng.randint(1, 70), rng.randint(1, 70) if rng.random() < 0.3 else 6))
        x, y, c = rng.randint(-200, 1200), rng.randint(-300, 1000), []
        for i in range(k):
            if not (i and rng.random() < 0.12):            # (else the same coordinates again; one of them stays now and then anyway)
                x += rng.choice((0, 0, rng.randint(-150, 150)))
                y += rng.choice((0, rng.randint(-150, 150)))
            c.append((x, y, rng.random() < 0.6))
        out.append(c)
    if sum(len(c) for c in out) > 200:
        out = out[:2]
    return out


def _separate(t, dx, dy, kw):
    """the tuple with its x and its y deltas packed apart: no run spans the two (fontTools asserts that none does)"""
    index, head, data = t
    pack = {k[6:]: v for k, v in kw.items() if k.startswith("delta_")}
    joint = G.pack_deltas(list(dx) + list(dy), **pack)
    assert data.endswith(joint)
    return index, head, data[:len(data) - len(joint)] + G.pack_deltas(list(dx), **pack) + G.pack_deltas(list(dy), **pack)


def _glyphs(rng, n_glyphs, n_axes, shared_peaks):
    """-> (entries, variation data, the glyph ids fontTools cannot read: a delta run spans x and y in their data or a descendant's)"""
    entries, datas, level, blind = [], [], [], set()
    for g in range(n_glyphs):
        r = rng.random()
        parents = [c for c in range(g) if level[c] is not None and level[c] < 3]
        if g == 0 or r < 0.62 or not parents:
            contours = _contours(rng)
            n = sum(len(c) for c in contours)
            entries.append(G.simple_entry(contours))
            level.append(0)
            tuples, shared = _tuples(rng, n_axes, shared_peaks, contours, n)
        elif r < 0.67:
            entries.append(b"")
            level.append(None)
            tuples, shared, n = ([], "none", 0)
        else:
            recs = []
            for _ in range(rng.randint(1, 3)):
                xf = rng.choice((None, None, rng.choice((0.5, 0.75, -1.0, 0.999)), tuple(rng.randint(-16384, 16384) / 16384 for _ in range(4))))
                recs.append((rng.choice(parents), rng.randint(-300, 300), rng.randint(-300, 300), xf))
            if any(c in blind for c, *_ in recs):
                blind.add(g)
            entries.append(G.composite_entry(recs))
            level.append(1 + max(level[c] for c, *_ in recs))
            n = len(recs)
            tuples, shared = _tuples(rng, n_axes, shared_peaks, None, n)
        if not tuples:
            datas.append(b"" if rng.random() < 0.5 else G.glyph_variations([]))
            continue
        pack = _pack(rng)
        made, joint, still = [], rng.random() < 0.1, rng.random() < 0.8
        for kw, dx, dy in tuples:
            shared_index = kw.pop("shared")
            # the x delta of the left phantom point (number n): fontTools moves the outline by it (it places a glyph by its left
            # side bearing), the reader does not look at it.  Most glyphs keep it 0; the others are not compared with fontTools
            numbers = (shared if kw["points"] == "shared" else kw["points"])
            for at in ([n] if numbers is None else [i for i, v in enumerate(numbers) if v == n]):
                if still:
                    dx[at] = 0
                elif dx[at]:
                    blind.add(g)
            made.append(G.tuple_of(dx, dy, shared=shared_index, **kw))
            if not joint:
                made[-1] = _separate(made[-1], dx, dy, kw)
            elif made[-1] != _separate(made[-1], dx, dy, kw):
                blind.add(g)
        datas.append(G.glyph_variations(made, shared_points=shared, **{k: v for k, v in pack.items() if k in ("words", "two_byte")},
                                        **({"run": pack["point_run"]})) if shared != "none" else G.glyph_variations(made))
    return entries, datas, blind


def _with_bounds(entries):
    """the entries with the bounding boxes fontTools computes for them, and their xMin: fontTools places a glyph by its left side
    bearing against the header's xMin, so a face it is to read like the reader states both truthfully (the reader looks at neither)"""
    import io
    import struct
    from fontTools.ttLib import TTFont
    glyf = TTFont(io.BytesIO(G.raw_font(entries, None)))["glyf"]
    out, x_min = [], {}
    for i, e in enumerate(entries):
        if e:
            g = glyf[f"g{i}"]
            g.recalcBounds(glyf)
            e = e[:2] + struct.pack(">hhhh", g.xMin, g.yMin, g.xMax, g.yMax) + e[10:]
            x_min[i] = g.xMin
        out.append(e)
    return out, x_min


class Face:
    def __init__(self, seed, n_glyphs):
        rng = random.Random(f"gvar/{seed}/{n_glyphs}")
        self.seed, self.n_axes, self.name = seed, 1 + seed % 3, f"gvar_{seed}_{n_glyphs}"
        shared = [_peak(rng, self.n_axes) for _ in range(rng.randint(1, 4))]
        for attempt in range(20):
            entries, datas, self.blind = _glyphs(rng, n_glyphs, self.n_axes, shared)
            entries, x_min = _with_bounds(entries)
            table = dict(shared_tuples=shared, n_axes=self.n_axes, long_offsets=rng.random() < 0.7)
            self.font = G.raw_font(entries, G.gvar_table(datas, **table), n_axes=self.n_axes, advances={i: 300 + 7 * i for i in range(n_glyphs)},
                                   bearings=x_min)
            # for fontTools: the same face without the data of the glyph ids it cannot read (self.blind: not compared)
            self.font_for_fonttools = G.raw_font(entries, G.gvar_table([b"" if g in self.blind else d for g, d in enumerate(datas)], **table),
                                                 n_axes=self.n_axes, bearings=x_min)
            # positions: an edge position on every axis, 2.14 values at the peaks and region edges of the face, and random ones
            marks = sorted({v for t in shared for v in t} | {8192, -8192, 5000, ONE, -ONE})
            self.positions = [[rng.choice(G.EDGE_POSITIONS)[0] for _ in range(self.n_axes)], [rng.choice(marks) for _ in range(self.n_axes)],
                              [rng.randint(-ONE, ONE) for _ in range(self.n_axes)]]
            if not any(self.positions[0]):
                self.positions[0][0] = ONE
            if all(self.work(c) <= MAX_WORK for c in self.positions):
                return
        raise AssertionError("no face within the cap")

    def work(self, coords):
        """the largest tuples x points of a glyph id, by the restatement's own run (MAX_WORK + 1 where a glyph id is malformed)"""
        worst, cur = [0], [0, 0]

        def trace(what, *d):
            if what == "glyph":
                cur[0], cur[1] = (d[3] if d[0] == "simple" else d[2]) + 4, 0
            elif what == "tuple":
                cur[1] += 1
                worst[0] = max(worst[0], cur[0] * cur[1])
        with _tracing(trace):
            ok = G.restate(self.font, coords)["ok"]
        t = G._Tables(self.font)
        # (an empty entry has no outline of its own: that is not malformed data)
        return worst[0] if all(v or t.glyph(g) is None for g, v in enumerate(ok)) else MAX_WORK + 1


def face(seed, n_glyphs=N_GLYPHS):
    return Face(seed, n_glyphs)


@contextlib.contextmanager
def _tracing(fn):
    G.TRACE = fn
    try:
        yield
    finally:
        G.TRACE = None


# ---- what a run reached --------------------------------------------------------------------------------------------------------

FEATURES = (["tuple_shared_peak", "tuple_embedded_peak", "tuple_intermediate", "tuple_plain", "tuple_private_points", "tuple_shared_points",
             "tuple_skipped", "tuple_applied", "tuple_scaled", "points_all", "points_count_one_byte", "points_count_two_bytes",
             "points_count_two_bytes_below_128"]
            + [f"point_run_{w}_{k}" for w in ("bytes", "words") for k in (1, 127, 128)]
            + [f"delta_run_{w}_{k}" for w in ("zero", "bytes", "words") for k in (1, 63, 64)]
            + ["touched_none", "touched_one", "touched_all", "touched_first_only", "touched_last_only", "infer_equal_coordinates_equal_deltas",
               "infer_equal_coordinates_unequal_deltas", "infer_below_the_pair", "infer_above_the_pair", "infer_at_the_low_end",
               "infer_at_the_high_end", "infer_between", "phantom_touched", "phantom_untouched", "numbers_past_the_phantom_points",
               "simple_1_contour", "simple_6_contours", "contour_of_1_point", "contour_of_64_or_more", "composite_depth_1", "composite_depth_2",
               "composite_depth_3", "composite_with_transform", "composite_without_transform", "glyph_without_tuples", "glyph_of_8_tuples"])


def features(f, coords):
    """{feature: the glyph ids (top-level walks) that reached it} at the position"""
    reach, state = {}, {"gid": 0, "tuples": 0, "own": True}

    def hit(name):
        reach.setdefault(name, set()).add(state["gid"])

    def trace(what, *d):
        if what == "tuple":
            state["tuples"] += state["own"]
            for v in d:
                hit(f"tuple_{v}")
        elif what == "point_count":
            hit("points_all" if d[0] == "all" else f"points_count_{d[0]}")
            if d[0] == "two_bytes" and d[1] < 128:
                hit("points_count_two_bytes_below_128")
        elif what in ("point_run", "delta_run"):
            hit(f"{what}_{d[0]}_{d[1]}")
        elif what == "infer":
            hit(f"infer_{d[0]}")
        elif what == "phantom":
            hit("phantom_touched" if d[0] else "phantom_untouched")
            if d[1]:
                hit("numbers_past_the_phantom_points")
        elif what == "contour":
            touched, length, first, last = d
            if touched == 0:
                hit("touched_none")
            elif touched == length:
                hit("touched_all")
            elif touched == 1:
                hit("touched_one")
                if length > 1 and first:
                    hit("touched_first_only")
                if length > 1 and last:
                    hit("touched_last_only")
            if length == 1:
                hit("contour_of_1_point")
            if length >= 64:
                hit("contour_of_64_or_more")
        elif what == "glyph":
            state["own"] = d[1] == 0
            if d[0] == "simple" and d[1] == 0:
                if d[2] in (1, 6):
                    hit(f"simple_{d[2]}_contour{'s' if d[2] > 1 else ''}")
            elif d[0] == "composite":
                hit("composite_with_transform" if d[3] else "composite_without_transform")
            if d[0] == "simple" and 1 <= d[1] <= 3:
                hit(f"composite_depth_{d[1]}")

    t = G._Tables(f.font)
    with _tracing(trace):
        for gid in range(t.n_glyphs):
            state.update(gid=gid, tuples=0, own=True)
            G.walk(t, list(coords), gid, 0, G.IDENTITY, [])
            if state["tuples"] in (0, 8):
                hit("glyph_of_8_tuples" if state["tuples"] else "glyph_without_tuples")
    return reach


# ---- the restatement over numbers that count their roundings ---------------------------------------------------------------------

@contextlib.contextmanager
def _swapped(module, **names):
    old = {k: getattr(module, k) for k in names}
    for k, v in names.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(module, k, v)


def tracked_restate(font, coords):
    """per glyph id the flat list of coordinates as charstring_fuzz_kit.Tracked values (the order of restate's `coords`)"""
    t = G._Tables(font)
    out = []
    with _swapped(G, f32=F.tracked, IDENTITY=tuple(F.tracked(v) for v in G.IDENTITY)), _swapped(V, f32=F.tracked):
        for gid in range(t.n_glyphs):
            cmds = []
            G.walk(t, list(coords), gid, 0, G.IDENTITY, cmds)
            flat = [v for _, c in cmds for v in c]
            assert all(isinstance(v, F.Tracked) for v in flat)
            out.append(flat)
    return out


def fonttools_flat(font, coords):
    """{glyph id: (kinds, flat coordinates)} from fontTools' glyph set at the normalised position, in restate's order"""
    cbs, _, _ = G.fonttools_callbacks(font, dict(zip(("wght", "wdth", "slnt", "opsz"), [c / 16384.0 for c in coords])), exact=False, normalized=True)
    out = {}
    for cp in sorted(cbs):
        kinds, flat = [], []
        for kind, x1, y1, x2, y2, x, y in cbs[cp]:
            kinds.append(kind)
            flat += [] if kind == G.Z else [x1, y1, x, y] if kind == G.Q else [x, y]
        out[cp - 0x100] = (kinds, flat)
    return out


# ---- one rule broken each --------------------------------------------------------------------------------------------------------

def _restate_with(module, name, *swaps):
    fn = F.variant(getattr(module, name), *swaps)

    def restate(font, coords):
        with _swapped(module, **{name: fn}):
            return G.restate(font, coords)
    return restate


def _advances_with(*swaps):
    fn = F.variant(P.phantom_sums, *swaps)

    def deltas(font, coords):
        with _swapped(P, phantom_sums=fn):
            return P.restate_deltas(font, coords)
    return deltas


# (rule, "outline" | "advance", restate(font, coords)): every one must disagree with the host reader somewhere in a corpus
def _outline(rule, module, name, *swaps):
    return rule, "outline", _restate_with(module, name, *swaps)


MUTANTS = [
    _outline("packed_point_run_of_127", G, "read_points",
             ("for _ in range((control & 0x7F) + 1):", "for _ in range(min((control & 0x7F) + 1, 127)):")),
    _outline("zero_run_deltas_skipped", G, "read_deltas", ("                out.append(0)\n", "                pass\n")),
    _outline("delta_run_of_63", G, "read_deltas",
             ("for _ in range((control & 0x3F) + 1):", "for _ in range(min((control & 0x3F) + 1, 63)):")),
    _outline("iup_equal_coordinates_take_the_first_delta", G, "infer", ("return da if da == db else f32(0)", "return da")),
    _outline("iup_outside_the_pair_takes_the_other_end", G, "infer", ("return da if pa < pb else db", "return db if pa < pb else da")),
    _outline("iup_wraps_to_the_wrong_neighbour", G, "accumulate", ("default=touched[-1])", "default=touched[0])")),
    _outline("intermediate_region_ignored", G, "accumulate",
             ("if index & 0x4000:\n            start = ", "h += 4 * n_axes if index & 0x4000 else 0\n        if False:\n            start = ")),
    _outline("axis_factor_from_the_wrong_side", V, "axis_factor",
             ("return f32(coord - start) / f32(peak - start)", "return f32(coord - start) / f32(end - start)")),
    ("phantom_point_n_plus_1", "advance", _advances_with(("            elif number == n + 1:\n", "            elif number == n + 2:\n"),
                                                         ("            if number == n:\n", "            if number == n + 1:\n"),
                                                         ("values[n + 1])", "values[n + 2])"), ("values[n])", "values[n + 1])"))),
    ("right_phantom_point_of_a_list_ignored", "advance", _advances_with(("            elif number == n + 1:\n", "            elif False:\n"))),
]


# ---- the comparisons the tests and tools/fuzz_decoders.py share --------------------------------------------------------------------

TABLE_KEYS = ("cmd_off", "dat_off", "kinds", "coords")


def host_views(vg, f, coords):
    """(the description for the device, the host reader's command table, its (deltas, states) of rule G7) of the face placed at coords"""
    mgr = vg.FontManager(False)
    mgr.set_gvar_advances(True)
    fid = mgr.add_font_instance_normalized("Fuzz", f.font, list(coords))
    return mgr.gvar_font_desc(fid), mgr.command_font_desc(fid), mgr.font_gvar_advance_deltas(fid)


def first_difference(f, coords, host, advances, restate=G.restate, restate_deltas=P.restate_deltas):
    """None where the host reader's table and advance deltas are the restatement's bit for bit; else a line that names the glyph
    id and the first differing record"""
    want = restate(f.font, coords)
    if not all(G.bits(host[k]) == G.bits(want[k]) for k in TABLE_KEYS):
        for g in range(len(want["cmd_off"]) - 1):
            a = [(int(k), c) for k, c in _records(host, g)]
            b = [(int(k), c) for k, c in _records(want, g)]
            if a != b:
                at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                return f"{f.name} at {list(coords)}: glyph id {g}, command {at}: host {a[at:at + 1]}, restatement {b[at:at + 1]}"
        return f"{f.name} at {list(coords)}: the offset arrays differ"
    d, state = restate_deltas(f.font, coords)
    if G.bits(advances[0]) != G.bits(d) or advances[1].tolist() != state.tolist():
        g = next(i for i in range(len(d)) if G.bits(advances[0][i:i + 1]) != G.bits(d[i:i + 1]) or advances[1][i] != state[i])
        return f"{f.name} at {list(coords)}: glyph id {g}, advance delta: host {advances[0][g]!r} ({advances[1][g]}), restatement {d[g]!r} ({state[g]})"
    return None


_FLOATS = {G.M: 2, G.L: 2, G.Q: 4, G.C: 6, G.Z: 0}


def _records(table, g):
    at = int(table["dat_off"][g])
    for kind in table["kinds"][table["cmd_off"][g]:table["cmd_off"][g + 1]]:
        n = _FLOATS[int(kind)]
        yield kind, np.asarray(table["coords"][at:at + n], np.float32).tobytes().hex()
        at += n
