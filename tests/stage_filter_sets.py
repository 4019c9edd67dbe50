"""Input sets aimed at the STAGE of the default raster kernel (csrc/sdf_span_kernel.inc): a segment's bracket of sample rows,
which it takes from the f32 record where the record fixes it and from first_ge in f64 where it does not, and a crossing's
column, which it takes from the f64 crossing ("The stage's integers").  Not a test module: imported by
tests/test_gpu_stage_filters.py, by its child process tests/stage_filter_child.py, by tests/test_stage_filter_model.py and by
tools/model_stage_filters.py.

Every set is deterministic; a glyph is (segs[n, 4], x0, y0, w, h).  A row centre is y0 + n + 1/2 and a column centre
x0 + k + 1/2; the rects are placed so that the centre under test is 1/2, where a double resolves an offset of 2^-52.

A wrong ROW adds or drops a crossing and flips the winding of the whole pixel row to the right of it: the inside and the outside
byte of a pixel differ wherever it lies 1/64 px or more from the outline, so the row shows.  A wrong COLUMN flips ONE pixel, the
one whose centre the crossing passed on the wrong side, and that pixel is as near to the segment as the crossing is to its
centre: only an error of 1/64 px or more can change a byte.  With u M = 2.4e-4 px at M = 4000 an f32 crossing is wrong by
1e-3 px at the most, so the column cases that caught the f32 column filter with its margin at 0 (built, measured and not kept)
sit at M = 9e5 (u M = 0.05 px); the ones at M = 4000 are kept as the edges they are.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

JS = tuple(range(10, 53))          # offsets 2^-j from a centre
JS_COARSE = tuple(range(10, 53, 3))


def ring(points):
    p = np.array([[float(x), float(y)] for x, y in points], dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def offsets(js):
    out = [Fraction(0)]
    for j in js:
        out += [Fraction(1, 2 ** j), -Fraction(1, 2 ** j)]
    return out


# ---- row_edge: a vertex at a row centre +- 2^-j and on it; the vertex is the end of one segment and the start of the next, and
# every ring comes in both orientations (its segments go up in one and down in the other): the half-open rule lo <= py < hi ----
def _row_glyph(d, far=0.0, rev=False, w=30, h=30, row=12, top=None):
    y0 = -row  # row `row` has its centre at 1/2
    x0 = -9
    p = (x0 + Fraction(41, 4), Fraction(1, 2) + d)
    f = Fraction(far)  # (the factors: far vertices that are no short binary fractions, or the f32 record would hold them exactly)
    q = (x0 + Fraction(103, 4) + f * Fraction(10007, 10000), y0 + Fraction(121, 4) + f * Fraction(7507, 10000))
    r = (x0 + Fraction(113, 4) - f * Fraction(1237, 10000), y0 + Fraction(21, 4) - f * Fraction(6173, 10000))
    if top is not None:  # q at `top` below 4096 above the bitmap's middle row (the origin of the f32 record)
        q = (q[0], y0 + h // 2 + 4096 - Fraction(top))
    pts = [p, q, r]
    return ring(pts[::-1] if rev else pts), x0, y0, w, h


def row_edge():
    return [_row_glyph(d, rev=rev) for d in offsets(JS) for rev in (False, True)]


# ---- col_edge: a vertical and a 3-4-5 slanted edge whose crossing of a row centre lies at a column centre +- 2^-j and on it, for
# column 0, a middle column and the last one (beyond it: the cell w, "no column left") ----
def _col_glyph(d, place, slant, far=0.0, w=24, h=24, rev=False, dirn=(3, 4)):
    col = {"first": 0, "mid": 7, "last": w - 1}[place]
    x0, y0 = -col, -10  # column `col` and row 10 have their centres at 1/2
    cx, cy = Fraction(1, 2) + d, Fraction(1, 2)
    f = Fraction(far) + (Fraction(1, 3) if far else 0)  # (a third: far ends that are no short binary fractions, each the nearest double)
    t1, t2 = 1 + f * Fraction(7, 8), 3 + f  # the crossing sits a quarter (far: about half) of the way along the edge
    if slant:
        a = (cx - dirn[0] * t1, cy - dirn[1] * t1)
        b = (cx + dirn[0] * t2, cy + dirn[1] * t2)
    else:
        a = (cx, cy - Fraction(27, 8) - 4 * f)
        b = (cx, cy + Fraction(61, 8) + 4 * f)
    c = (x0 + (Fraction(71, 4) if place != "last" else Fraction(13, 4)), y0 + Fraction(47, 4))
    pts = [a, b, c]
    return ring(pts[::-1] if rev else pts), x0, y0, w, h


def col_edge():
    return [_col_glyph(d, place, slant) for d in offsets(JS_COARSE) for place in ("first", "mid", "last") for slant in (False, True)]


# ---- flat: |dy| = 2^-20 .. 2^-40 with |dx| up to w, across one row centre: E_xc is huge, first_ge must give the column ----
def flat():
    out = []
    w, h = 32, 24
    x0, y0 = -3, -10
    for j in range(20, 41):
        for dx in (Fraction(13, 4), Fraction(w - 5)):
            for rev in (False, True):
                dy = Fraction(1, 2 ** j)
                a = (x0 + Fraction(9, 4), Fraction(1, 2) - dy / 2)
                b = (a[0] + dx, Fraction(1, 2) + dy / 2)
                c = (x0 + Fraction(37, 4), y0 + Fraction(81, 4))
                pts = [a, b, c]
                out.append((ring(pts[::-1] if rev else pts), x0, y0, w, h))
    return out


# ---- far: the edges of row_edge and col_edge extended past the window ----
FAR_4000 = 4000


def far_row():
    """M = 4000.  The near vertex P is v + d of the record of the segment that arrives from the far vertex Q, and v + d lands on
    the wrong side of P's row centre only where d = P - Q lies in a higher binade than v = Q - origin: v + d is then a multiple
    of ulp(v) = 2^-13 px and the two roundings add up to 1.5 of it.  So Q lies 0.1 .. 2.4 px below 4096 above the origin, P
    2.5 px below the origin, and every glyph has its own Q (one draw of the roundings each)."""
    out = []
    for i, d in enumerate(offsets(JS)):
        top = Fraction(1 + (37 * i) % 23, 10) + Fraction(1, 3000)
        out += [_row_glyph(d, far=FAR_4000 - 13 * i, rev=rev, top=top) for rev in (False, True)]
    return out


def far_col_4000():
    return [_col_glyph(d, "mid", slant, far=FAR_4000 - 29 * i, rev=rev) for i, d in enumerate(offsets(JS_COARSE)) for slant in (False, True)
            for rev in (False, True)]


# (t2 of the slanted edge, M = 4 t2 = 8.7e5 .. 9.6e5, below the 10^6 of `sane`; offsets of the crossing in 1/128 px.  Chosen with
# tools/model_stage_filters.py: at each t2 the un-margined f32 column differs from first_ge's for a pixel 1/64 px or more from the
# edge, whichever of the three reciprocals within 1 ulp v_rcp_f32 returns)
FAR_COL_BIG = (239000, 235012, 234015, 229030, 222051, 217066)
FAR_COL_BIG_D = (3, -3, 4, -4, 5, -5, 6, -6)


def far_col_big():
    """3-4-5 edges through a column centre +- 3/128 .. 6/128 px, extended to M = 9e5 (u M = 0.05 px): the f32 crossing is off by
    hundredths of a pixel, and the pixel whose winding a wrong column flips lies 1/64 px or more from the edge"""
    return [_col_glyph(Fraction(d, 128), "mid", True, far=t2, rev=rev) for t2 in FAR_COL_BIG for d in FAR_COL_BIG_D for rev in (False, True)]


def far_col():
    return far_col_4000() + far_col_big()


def far_insane():
    """just above M = 10^6: `sane` is off, and so is every f32 decision of the stage"""
    return [_row_glyph(Fraction(1, 2 ** 30), far=1000100, rev=rev) for rev in (False, True)] + \
           [_col_glyph(Fraction(1, 2 ** 30), "mid", True, far=250100, rev=rev) for rev in (False, True)]


# ---- walk: 64 near-vertical segments, each across 35 rows of a 16 x 40 bitmap: 2240 (segment, row) pairs in one wave, above the
# 256 of the pool, so every thread walks its own rows; the second half pins some of the segments to a column centre +- 2^-j ----
def _walk_glyph(d=None):
    w, h = 16, 40
    x0, y0 = -7, -20
    pts = []
    for i in range(32):
        x = x0 + Fraction(3, 2) + Fraction(i * 3, 8)
        xb = xt = x
        if d is not None and i % 4 == 0:
            xb = xt = x0 + i // 4 + 4 + Fraction(1, 2) + d  # exactly vertical at a column centre + d
        elif d is not None and i % 4 == 2:
            xb, xt = x - Fraction(3, 64), x + Fraction(3, 64)
        pts.append((xb, y0 + Fraction(9, 4)))
        pts.append((xt + Fraction(1, 8), y0 + Fraction(151, 4)))
    return ring(pts), x0, y0, w, h


def walk():
    return [_walk_glyph()] + [_walk_glyph(d) for d in offsets((10, 17, 24, 31, 38, 45, 52))]


# ---- partial: glyphs whose last chunk of 256 records holds 1, 7, 8 and 9 of them (and glyphs of that many segments), the long
# member of the last group of eight being its last record, away from the group's anchor ----
def _partial_glyph(n, seed):
    rng = np.random.default_rng(seed)
    w = h = 40
    x0, y0 = -20, -20
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n - 1))
    rad = 13.0 + rng.uniform(-0.4, 0.4, n - 1)
    pts = [(float(r * np.cos(a)), float(r * np.sin(a))) for a, r in zip(ang, rad)]
    pts.append((17.25, -16.5))  # the last record runs from here back to the first vertex: the long one
    return ring(pts), x0, y0, w, h


def partial():
    return [_partial_glyph(n, 7 * n) for n in (1 + 2, 7, 8, 9, 256 + 1, 256 + 7, 256 + 8, 256 + 9, 512 + 1, 512 + 9)]


# ---- wide_rows: w = 3, 255, 256, 257 with spans of 1 .. 4 tiles (a tile: 256 pixels in row order) ----
def wide_rows():
    out = []
    for w in (3, 255, 256, 257):
        for tiles in (1, 2, 3, 4):
            npix = 256 * tiles - (0 if tiles == 1 and w == 256 else 37)
            h = max(1, -(-npix // w)) if w > 3 else max(1, npix // w)
            x0, y0 = -(w // 2), -(h // 2)
            pts = [(x0 + 0.75, y0 + 0.25), (x0 + w - 0.5, y0 + 0.5 * h + 0.125), (x0 + 0.4 * w + 0.3, y0 + h - 0.25),
                   (x0 + 0.5 * w, y0 + 0.5 * h + 0.0625)]
            out.append((ring(pts), x0, y0, w, h))
    return out


# ---- fuzz: 300 random small glyphs from a fixed seed; a third of them on the half-pixel grid, where centres are hit exactly ----
def fuzz():
    rng = np.random.default_rng(0x57A6E)
    out = []
    for i in range(300):
        w, h = int(rng.integers(3, 41)), int(rng.integers(3, 41))
        x0, y0 = int(rng.integers(-60, 20)), int(rng.integers(-60, 20))
        n = int(rng.integers(3, 25))
        p = np.stack([rng.uniform(x0 - 3, x0 + w + 3, n), rng.uniform(y0 - 3, y0 + h + 3, n)], 1)
        if i % 3 == 0:
            p = np.round(p * 2.0) / 2.0
        elif i % 3 == 1:
            k = rng.integers(0, n)
            p[k] = np.floor(p[k]) + 0.5 + rng.choice([-1.0, 1.0], 2) * 2.0 ** -float(rng.integers(10, 50))
        out.append((ring(p), x0, y0, w, h))
    return out


@lru_cache(maxsize=None)
def sets():
    """name -> list of glyphs"""
    return {"row_edge": row_edge(), "col_edge": col_edge(), "flat": flat(), "far_row": far_row(), "far_col": far_col(),
            "far_insane": far_insane(), "walk": walk(), "partial": partial(), "wide_rows": wide_rows(), "fuzz": fuzz()}
