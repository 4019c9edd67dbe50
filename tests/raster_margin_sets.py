"""Input sets aimed at the numerical MARGINS of the default raster kernel, not a test module.

Imported by tests/test_raster_margin_sets_host.py (CPU: oracle == numpy restatement, witnesses), by
tests/test_gpu_raster_margins.py (product variants 0 and 1) and by that test's child process (the margins build:
`make margins`, csrc/sdf_margin_kernels.hip).  Every set is deterministic; a glyph is (segs[n,4], x0, y0, w, h).

Geometry used throughout: an edge along a Pythagorean direction (a, b) / c with vertices on a dyadic grid has the
EXACT rational distance |b px - a py - C| / c to a pixel centre, and the pixels of the lattice lines b i - a j = N0 + c k
all sit at k + (2 m + 1) / 64 + eps from it: a whole family of pixels at a controlled eps from a rounding boundary of the
byte (32 d + 1/2 an integer, renderer_precise.rs:75-79), on one side of the edge at +eps and on the other at -eps, while
the f32 filter really rounds (3/5, 4/5, 5/13 ... are not dyadic).
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

PYTH = ((4, 3, 5), (12, 5, 13), (15, 8, 17))


class MarginSet:
    def __init__(self, name, glyphs, eps=None, per_wave=None, near=False, M=None):
        self.name = name
        self.glyphs = glyphs
        self.eps = eps            # per glyph: |eps| of its near-boundary pixels (None: no such tier)
        self.per_wave = per_wave  # near-boundary pixels every occupied 64-pixel wave of the tile order holds
        self.near = near          # the set is a near-boundary set (every tier holds >= 64 witness pixels)
        self.M = M                # coordinate bound of its chunks, about


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def bbox_rect(segs, margin=3):
    lo = np.floor(segs[:, [0, 1]].min(0)).astype(np.int64) - margin
    hi = np.ceil(segs[:, [0, 1]].max(0)).astype(np.int64) + margin
    return segs, int(lo[0]), int(lo[1]), int(hi[0] - lo[0]), int(hi[1] - lo[1])


def min_dist(segs, x0, y0, w, h):
    """numpy f64 distance field in the reference's operation order (segment.rs:54-72, point.rs:38-42): [h, w], top row first"""
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    px = (np.arange(w, dtype=np.float64) + (np.float64(x0) + 0.5))[None, :]
    py = (np.arange(h, dtype=np.float64) + (np.float64(y0) + 0.5))[:, None]
    best = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for vx, vy, wx, wy in segs:
            dx, dy = wx - vx, wy - vy
            l2 = dx * dx + dy * dy
            t = ((px - vx) * dx + (py - vy) * dy) / l2
            qx, qy = vx + t * dx, vy + t * dy
            at_v = (l2 == 0.0) | (t < 0.0)
            qx = np.where(at_v, vx, np.where(t > 1.0, wx, qx))
            qy = np.where(at_v, vy, np.where(t > 1.0, wy, qy))
            ex, ey = qx - px, qy - py
            best = np.minimum(best, ex * ex + ey * ey)
    return np.sqrt(best)[::-1]


def boundary_offset(d):
    """|32 d + 1/2 - nearest integer| per pixel"""
    s = 32.0 * d + 0.5
    return np.abs(s - np.rint(s))


def witness_count(glyph, eps):
    return int((boundary_offset(min_dist(*glyph)) <= 32.0 * 2.0 * abs(eps)).sum())


def wave_counts(glyph, eps):
    """near-boundary pixels per 64-pixel wave of the tile order (pixel index = row * w + x, top row first)"""
    near = (boundary_offset(min_dist(*glyph)) <= 32.0 * 2.0 * abs(eps)).ravel()
    pad = (-near.size) % 64
    return np.concatenate([near, np.zeros(pad, bool)]).reshape(-1, 64).sum(1)


# ---------------------------------------------------------------------------------------------------------------
# exact placement of a Pythagorean edge
# ---------------------------------------------------------------------------------------------------------------
def _egcd(a, b):
    if b == 0:
        return a, 1, 0
    g, x, y = _egcd(b, a % b)
    return g, y, x - (a // b) * y


def _exact(fr):
    f = float(fr)
    assert Fraction(f) == fr, f"{fr} is not a double"
    return f


def pyth_point(abc, rect0, centre, m, eps):
    """A dyadic point (Fractions) of the line with direction (a, b) that passes next to `centre`, such that the pixel
    centres of the lattice lines b i - a j = N0 + c k (pixel (i, j) of the bitmap with origin rect0) lie at the signed
    distance k + (2 m + 1) / 64 + eps on the side of the normal (b, -a) / c."""
    a, b, c = abc
    X0, Y0 = rect0
    eps = Fraction(eps)
    cx, cy = Fraction(centre[0]), Fraction(centre[1])
    off = Fraction(b - a, 2) + b * X0 - a * Y0                 # b px - a py of pixel (i, j) = N + off
    target = b * cx - a * cy
    N0 = round(target + c * Fraction(2 * m + 1, 64) - off)
    Cc = N0 + off - c * (Fraction(2 * m + 1, 64) + eps)        # b x - a y = Cc on the line
    s = Cc.denominator                                          # a power of two
    assert s & (s - 1) == 0
    K = Cc.numerator
    g, u, v = _egcd(b, a)                                       # b u + a v = 1
    assert g == 1
    X, Y = K * u, -K * v                                        # b X - a Y = K
    t = round((Fraction(X, s) - cx) / a)
    X, Y = X - a * t * s, Y - b * t * s
    return Fraction(X, s), Fraction(Y, s)


def pyth_triangle(abc, rect, m, eps, L, Lq, sub=0, centre=None, along=0, exact=True):
    """ring (P-, P+, [subdivided] Q): the long edge P- -> P+ = Pc -+ L (a, b) through the window `rect`, closed through
    Q = Pc + Lq (b, -a); `sub` > 0 splits the two closing edges into that many pieces each (a power of two)"""
    a, b, c = abc
    x0, y0, w, h = rect
    centre = centre or (x0 + w // 2, y0 + h // 2)
    pcx, pcy = pyth_point(abc, (x0, y0), centre, m, eps)
    pcx, pcy = pcx + Fraction(along) * a, pcy + Fraction(along) * b
    L, Lq = Fraction(L), Fraction(Lq)
    pm = (pcx - L * a, pcy - L * b)
    pp = (pcx + L * a, pcy + L * b)
    q = (pcx + Lq * b, pcy - Lq * a)
    pts = [pm, pp]
    for p0, p1 in ((pp, q), (q, pm)):
        n = max(sub, 1)
        for k in range(1, n + 1):
            pts.append((p0[0] + (p1[0] - p0[0]) * k / n, p0[1] + (p1[1] - p0[1]) * k / n))
    pts = pts[:-1]  # the last point is P- again
    if not exact:  # eps below what the vertices resolve: each takes the nearest double
        return ring([(float(px), float(py)) for px, py in pts])
    return ring([(_exact(px), _exact(py)) for px, py in pts])


# ---------------------------------------------------------------------------------------------------------------
# near-boundary sets
# ---------------------------------------------------------------------------------------------------------------
def _near_set(name, ladder, scale, rect=(0, 0, 40, 40), sub=0, M=None, exact=True):
    """per tier 2^-j and sign: one glyph per Pythagorean direction; the long edge reaches `scale` px from the window's middle"""
    glyphs, eps = [], []
    for n, j in enumerate(ladder):
        for sign in (1, -1):
            for d, abc in enumerate(PYTH):
                e = sign * Fraction(1, 2 ** j)
                L = Fraction(int(scale * 16 / max(abc[:2])), 16) if scale < 64 else int(scale / max(abc[:2]))
                # end points at a generic position ALONG the line (the line itself stays put): their f32 records round
                segs = pyth_triangle(abc, rect, (5 * n + 3 * d) % 32, e, L, L / 2 if scale >= 64 else L, sub=sub,
                                     along=Fraction(0x2E9E3 + 0x1357 * (n + d), 2 ** 18) - Fraction(1, 2), exact=exact)
                glyphs.append((segs,) + tuple(rect))
                eps.append(float(abs(e)))
    return MarginSet(name, glyphs, eps=eps, near=True, M=M or scale)


LADDER = (10, 13, 16, 20, 24, 28, 32, 36, 40, 44)   # eps = 2^-j, placed EXACTLY: from 1e-3 px to 6e-14 px = 16 ulp of a 32 px coordinate
# ... and on below the f64 resolution: ulp(32 d + 1/2) is 2^-47 .. 2^-45 for d = 1 .. 6 px, i.e. 2^-52 .. 2^-50 px.  A window
# around the origin; the vertices take the nearest double (eps is below what they resolve: 2^-49 at 8 px), so the side of the
# boundary a pixel lands on is decided by the roundings of the placement and of the reference's own f64 arithmetic
LADDER_SUB = (46, 48, 50, 52, 53, 56)
LADDER_M = (10, 12, 14, 16, 20, 24, 28)             # (the far vertices leave 2^-30 of a coordinate at M = 10^6)
LADDER_ABS = (10, 14, 18, 22, 26)                   # (2^-29 at an origin of 2^24)


def near_boundary():
    return _near_set("near_boundary", LADDER, 20)


def near_subulp():
    return _near_set("near_subulp", LADDER_SUB, 20, rect=(-20, -20, 40, 40), exact=False)


def near_M(tag, scale):
    return _near_set(f"near_M{tag}", LADDER_M, scale, sub=32, M=scale)


def abs_position():
    glyphs, eps = [], []
    for T in (2 ** 23, 2 ** 24 - 64):
        s = _near_set("", LADDER_ABS, 20, rect=(T, T, 40, 40))
        glyphs += s.glyphs
        eps += s.eps
    return MarginSet("abs_position", glyphs, eps=eps, near=True, M=20)


# ---------------------------------------------------------------------------------------------------------------
# undecided-lane counts: w = 64, so a wave of the tile order is one row of the bitmap
# ---------------------------------------------------------------------------------------------------------------
LANES_EPS = 2.0 ** -30


def lanes(n_per_wave):
    """n small triangles side by side, 20 px apart (a multiple of c = 5: the same lattice lines), each with one short
    3-4-5 edge of length 3.75 (two pixels of one row on near-boundary lattice lines are 4 apart along the edge): a row
    of the bitmap holds one near-boundary pixel per triangle, or none"""
    glyphs = []
    for m in (0, 7, 19, 30):
        base = pyth_triangle(PYTH[0], (0, 0, 64, 16), m, Fraction(1, 2 ** 30), Fraction(3, 8), Fraction(3, 4), centre=(10, 8),
                             along=Fraction(1, 16))
        segs = np.concatenate([base + np.array([20.0 * k, 0.0, 20.0 * k, 0.0]) for k in range(n_per_wave)])
        glyphs.append((segs, 0, 0, 64, 16))
    return MarginSet(f"lanes_{n_per_wave}", glyphs, eps=[LANES_EPS] * len(glyphs), per_wave=n_per_wave, M=33)


def lanes_row():
    """axis-parallel box reaching past the window on both sides: every pixel of every row is near-boundary"""
    glyphs = []
    for m in (0, 11, 26):
        o = (2 * m + 1) / 64.0 + LANES_EPS
        glyphs.append((ring([(-10.0, 4.5 - o), (74.0, 4.5 - o), (74.0, 11.5 + o), (-10.0, 11.5 + o)]), 0, 0, 64, 16))
    return MarginSet("lanes_row", glyphs, eps=[LANES_EPS] * len(glyphs), per_wave=64, M=43)


# ---------------------------------------------------------------------------------------------------------------
# argmin swaps: the f32 argmin is not the f64 argmin
# ---------------------------------------------------------------------------------------------------------------
def argmin_swap():
    """Two rings with one long edge each on two parallel lines 2^-30 apart: edge A at (boundary - 2^-31) from its lattice
    pixels, edge B (other end points, other length: another f32 record) at (boundary + 2^-31): A is the nearest
    segment and decides the byte, the f32 filter values of A and B differ by their own roundings only.  Plus corners
    where two edges meet at a shallow angle."""
    glyphs = []
    rect = (0, 0, 40, 40)
    for d, abc in enumerate(PYTH):
        for m in (2 + d, 17 + d):
            L = Fraction(int(20 * 16 / max(abc[:2])), 16)
            ea = pyth_triangle(abc, rect, m, -Fraction(1, 2 ** 31), L, L)
            eb = pyth_triangle(abc, rect, m, Fraction(1, 2 ** 31), L - Fraction(1, 8), L + Fraction(1, 4), along=Fraction(3, 16))
            glyphs.append((np.concatenate([ea, eb]),) + rect)
    for k, ang in enumerate((2.0 ** -12, 2.0 ** -16, 2.0 ** -20)):
        # a corner at (20.25, 20 + 1/64): the two edges leave it at +-ang against the x axis
        c = (20.25, 20.0 + (2 * k + 1) / 64.0)
        glyphs.append((ring([c, (2.0, c[1] + 18.25 * ang), (2.0, 3.0), (38.0, 3.0), (38.0, c[1] + 17.75 * ang)]),) + rect)
    return MarginSet("argmin_swap", glyphs, eps=[2.0 ** -31] * 6 + [None] * 3, M=20)


# ---------------------------------------------------------------------------------------------------------------
# candidate rule: r_g, SAT, far
# ---------------------------------------------------------------------------------------------------------------
def cand_long_in_group():
    """16 segments = 2 groups of 8 records.  Group 0: five tiny segments at the far end (the anchor is the start of
    member 4), ONE long segment, two tiny ones at its near end: the nearest point of the group lies up to `length` px from
    its anchor, and only r_g keeps the group a candidate for the pixels along the long segment.  Group 1 closes the ring."""
    glyphs = []
    for length, flip in ((6.0, False), (9.75, False), (12.0, True), (7.5, True)):
        x = [2.0 + 0.05 * k for k in range(6)] + [2.25 + length, 2.3 + length, 2.35 + length]
        pts = [(v, 10.0) for v in x]                                     # segments 0..7 (group 0), left to right
        xe = x[-1]
        pts += [(xe, 10.0 + 0.05 * k) for k in range(1, 5)]              # segments 8..11 (tiny, upwards); member 12 starts here
        pts += [(xe, 14.0), (2.0, 14.0), (2.0, 10.05)]                   # segments 12..15 back to the start
        p = np.array(pts)
        if flip:
            p = np.stack([p[:, 1] - 8.0, p[:, 0] + 2.0], 1)[::-1]
            p = np.roll(p, 1, axis=0)
        glyphs.append(bbox_rect(ring(p), 5))
    return MarginSet("cand_long_in_group", glyphs, M=12)


_F = np.float32


def _fma(a, b, c):
    return _F(np.float64(a) * np.float64(b) + np.float64(c))


def phase1_residuals(glyph, pixel):
    """The kernel's phase-1 candidate test for `pixel` (column, row from the bottom) WITHOUT its inflations (INFL = 1, pad = 0,
    1.004 -> 1), restated in numpy f32 for a glyph of one chunk: per group of 8 records (U + r_g)^2 - D_g^2 as the kernel forms
    it (f32 records relative to the middle of the bitmap, anchor = start of member 4, D_g^2 truncated to its upper 16 bits).
    Negative: the group is not a candidate."""
    segs, x0, y0, w, h = glyph
    ox, oy = float(x0 + w // 2), float(y0 + h // 2)
    fvx, fvy = (segs[:, 0] - ox).astype(_F), (segs[:, 1] - oy).astype(_F)
    fdx, fdy = (segs[:, 2] - segs[:, 0]).astype(_F), (segs[:, 3] - segs[:, 1]).astype(_F)
    rpx, rpy = _F(pixel[0] - w // 2) + _F(0.5), _F(pixel[1] - h // 2) + _F(0.5)
    groups = []
    for g0 in range(0, len(segs), 8):
        ai = min(g0 + 4, len(segs) - 1)
        ax, ay = fvx[ai], fvy[ai]
        r2 = _F(0)
        for i in range(g0, min(g0 + 8, len(segs))):
            wx, wy = _F(fvx[i] + fdx[i]), _F(fvy[i] + fdy[i])
            ex, ey, fx, fy = _F(fvx[i] - ax), _F(fvy[i] - ay), _F(wx - ax), _F(wy - ay)
            r2 = max(r2, _fma(ey, ey, _F(ex * ex)), _fma(fy, fy, _F(fx * fx)))
        ddx, ddy = _F(rpx - ax), _F(rpy - ay)
        groups.append((_F(np.sqrt(r2)), _fma(ddy, ddy, _F(ddx * ddx))))
    U = min(_F(np.sqrt(min(d2 for _, d2 in groups))), _F(6.2))
    out = []
    for r, d2 in groups:
        tt = _F(U + r)
        d2t = (np.array([d2], dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)[0]
        out.append(float(_fma(tt, tt, -d2t)))
    return out


EQUALITY_PIXEL = (8, 8)
EQUALITY_DELTA = 2.0 ** -16
# (direction, n, offset, m): the far anchor lies at D = 256 sqrt(n) + offset from the pixel (D^2 just above a number whose
# lower 16 bits are zero: the truncation of D_g^2 gives nothing away), the boundary is (2 m + 1) / 64.  Chosen with
# phase1_residuals among 648 such placements: the 30 whose group 0 fails the test without inflations.
_EQUALITY = ((0, 137, 2e-05, 141), (0, 151, 2e-05, 115), (0, 172, 6e-05, 115), (0, 186, 2e-05, 115), (0, 193, 2e-05, 141),
             (0, 200, 6e-05, 115), (0, 207, 2e-05, 128), (0, 228, 2e-05, 115), (1, 137, 2e-05, 141), (1, 172, 2e-05, 115),
             (1, 186, 2e-05, 115), (1, 193, 2e-05, 141), (1, 200, 6e-05, 141), (1, 228, 6e-05, 141), (1, 249, 2e-05, 115),
             (2, 137, 2e-05, 141), (2, 172, 2e-05, 115), (2, 186, 2e-05, 115), (2, 193, 2e-05, 141), (2, 200, 6e-05, 141),
             (2, 228, 6e-05, 141), (2, 249, 2e-05, 115), (3, 137, 2e-05, 141), (3, 151, 2e-05, 115), (3, 172, 6e-05, 115),
             (3, 186, 2e-05, 115), (3, 193, 2e-05, 141), (3, 200, 6e-05, 115), (3, 207, 2e-05, 128), (3, 228, 2e-05, 115))


def cand_equality():
    """The candidate rule D_g <= U + r_g at EQUALITY, where only the inflations of phase 1 (INFL, pad, 1.004) cover the f32
    roundings.  16 x 16 window, pixel p = (8.5, 8.5), unit direction u.  Group 0 (8 records): a tiny loop at its anchor a_g =
    p - D u, ~3500 px away (f32 coordinates there are 2.4e-4 px apart), and ONE long segment a_g -> q that points straight
    at the pixel and ends at q = p - (b - delta / 2) u: p, q, a_g are collinear, D_g = |p - q| + r_g.  Group 1: a tiny ring
    whose nearest point to p is its anchor a' = p + (b + delta / 2) u, so U = |p - a'| = |p - q| + delta: the rule holds by
    delta = 2^-16 px.  b is a rounding boundary of the byte: q (group 0) gives one byte, a' another."""
    dirs = ((0.8, 0.6), (-0.6, 0.8), (0.6, -0.8), (-0.8, -0.6))
    glyphs = []
    for ui, n, off, m in _EQUALITY:
        u = np.array(dirs[ui])
        nrm = np.array([-u[1], u[0]])
        p = np.array([8.5, 8.5])
        b = (2 * m + 1) / 64.0
        ag, q, ap = p - (256.0 * np.sqrt(n) + off) * u, p - (b - EQUALITY_DELTA / 2) * u, p + (b + EQUALITY_DELTA / 2) * u
        loop = [ag, ag - 0.1 * u, ag - 0.1 * u + 0.1 * nrm, ag + 0.1 * nrm, ag]
        g0 = [(loop[i], loop[i + 1]) for i in range(4)] + [(ag, q), (q, ag), (ag, ag - 0.05 * nrm), (ag - 0.05 * nrm, ag)]
        offs = ((0.2, 0.1), (0.3, 0.1), (0.3, 0.05), (0.1, 0.05), (0.0, 0.0), (0.1, -0.05), (0.3, -0.05), (0.2, -0.1))
        v = [ap + s * u + t * nrm for s, t in offs]
        g1 = [(v[i], v[(i + 1) % 8]) for i in range(8)]
        glyphs.append((np.array([[a[0], a[1], c[0], c[1]] for a, c in g0 + g1]), 0, 0, 16, 16))
    return MarginSet("cand_equality", glyphs, M=3300)


def cand_sat_far():
    """finely flattened small shapes in wide windows: minima at 3 - 5.9 px outside (between the weakened SAT / far
    thresholds and the saturation distance 5.97 px) and 1 - 2 px inside, every group a fraction of a pixel long"""
    glyphs = []
    for r, n, c in ((3.0, 64, (12.3, 12.1)), (2.5, 256, (11.7, 12.45))):
        a = np.linspace(0, 2 * np.pi, n, endpoint=False)
        glyphs.append((ring(np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)), 0, 0, 24, 24))
    a = np.linspace(0, 2 * np.pi, 128, endpoint=False)
    outer = np.stack([16.2 + 6 * np.cos(a), 15.8 + 6 * np.sin(a)], 1)
    inner = np.stack([16.2 + 2 * np.cos(a), 15.8 + 2 * np.sin(a)], 1)[::-1]
    glyphs.append((np.concatenate([ring(outer), ring(inner)]), 0, 0, 32, 32))
    return MarginSet("cand_sat_far", glyphs, M=17)


# ---------------------------------------------------------------------------------------------------------------
# chunk boxes (glyphs of >= 3 chunks of 256 segments)
# ---------------------------------------------------------------------------------------------------------------
def _sliver(x_lo, x_hi, y_top, thick=0.2):
    """thin horizontal ring of exactly 256 segments: 127 along the top, 1, 127 along the bottom, 1"""
    xs = np.linspace(x_lo, x_hi, 128)
    top = np.stack([xs[::-1], np.full(128, y_top)], 1)
    bot = np.stack([xs, np.full(128, y_top - thick)], 1)
    return ring(np.concatenate([top, bot]))


def box_reach():
    """w = 32, h = 64: two spans of 32 rows; the upper one samples y = 32.5 .. 63.5.  Chunk 0 is a sliver `gap` below that
    band (its box strictly outside it): for the band's lowest rows it holds the nearest segment (gap 1.6), or sits just
    inside / just outside the skip's reach R = SAT + pad (gaps 6.19 / 6.25).  Chunk 1: a sliver near the top; chunk 2: a
    small triangle near the bottom."""
    glyphs = []
    for gap in (1.6, 6.19, 6.25):
        segs = np.concatenate([_sliver(4.0, 28.0, 32.5 - gap), _sliver(5.0, 27.0, 58.3), ring([(10.0, 4.0), (20.0, 4.5), (15.0, 8.0)])])
        assert len(segs) == 515
        glyphs.append((segs, 0, 0, 32, 64))
    return MarginSet("box_reach", glyphs, M=33)


def box_band():
    """a rectangle whose left side (chunk 0: 256 segments at x = -12, far outside the 20 x 20 window in x, but crossing
    every sample row) carries the winding number of the window's pixels"""
    glyphs = []
    for xl in (-12.0, -40.0):
        ys = np.linspace(16.0, 4.0, 257)
        left = np.stack([np.full(257, xl), ys], 1)                         # 256 segments, downwards
        ysr = np.linspace(4.0, 16.0, 257)
        right = np.stack([np.full(257, 10.0), ysr], 1)                     # bottom edge, then 256 segments upwards
        glyphs.append((ring(np.concatenate([left, right])), 0, 0, 20, 20))  # + the top edge: 514 segments
        assert len(glyphs[-1][0]) == 514
    return MarginSet("box_band", glyphs, M=50)


# ---------------------------------------------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------------------------------------------
def guard_huge():
    """segments longer than 10^15 px through the window: |d|^2 >= 10^30, the f32 record carries no usable 1 / |d|^2 (the
    filter value is the distance to the START vertex); only the `sane` guard keeps the filter away from them"""
    glyphs = [
        (ring([(-2.0e15, 10.3), (2.0e15, 10.3), (2.0e15, -3.0e15), (-2.0e15, -3.0e15)]), 0, 0, 20, 20),
        (ring([(-2.0e15, -1.5e15 + 10.0), (2.0e15, 1.5e15 + 10.0), (2.0e15, -3.0e15)]), 0, 0, 20, 20),
    ]
    return MarginSet("guard_huge", glyphs, M=2e15)


# ---------------------------------------------------------------------------------------------------------------
# the two directed generators of tools/fuzz_gpu.py (which imports them from here), seeded, fixed count
# ---------------------------------------------------------------------------------------------------------------
def boundary_glyph(rng):
    """rectilinear / nearly rectilinear polygons on the 1/64 px grid"""
    size = int(rng.choice([12, 24, 40, 80]))
    segs = []
    for k in range(int(rng.integers(1, 4))):
        x0, y0 = rng.integers(0, size * 64 // 2, 2)
        w, h = rng.integers(64, size * 64 // 2 + 65, 2)
        # odd multiples of 1/64 put pixel centres (k + 1/2) at distances (2 m + 1) / 64 from the edge: byte boundaries
        x0, y0, w, h = (int(v) | 1 for v in (x0, y0, w, h))
        pts = np.array([(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)], dtype=np.float64) / 64.0
        if rng.random() < 0.5:  # steps along one side: many collinear segments, ties between neighbours
            n = int(rng.integers(2, 200))
            xs = np.linspace(pts[0, 0], pts[1, 0], n + 1)[1:-1]
            xs = np.round(xs * 64) / 64
            pts = np.concatenate([pts[:1], np.stack([xs, np.full_like(xs, pts[0, 1])], 1), pts[1:]])
        if rng.random() < 0.3:  # a slight tilt: distances drift across the boundary along the edge
            pts[:, 1] += (pts[:, 0] - pts[0, 0]) * float(rng.choice([1, 2, 3])) / 4096.0
        if k % 2:
            pts = pts[::-1]
        segs.append(ring(pts))
    segs = np.concatenate(segs) + float(rng.choice([0.0, 0.0, 17.0, -300.0]))
    lo = np.floor(segs[:, [0, 1]].min(0)).astype(np.int64) - 3
    hi = np.ceil(segs[:, [0, 1]].max(0)).astype(np.int64) + 3
    return segs, int(lo[0]), int(lo[1]), int(hi[0] - lo[0]), int(hi[1] - lo[1])


def guard_glyph(rng):
    """a window of ~40 px on the near corner of an outline whose far vertices lie ~4096 px or ~10^6 px away"""
    far = float(rng.choice([4096.0, 4096.0, 1.0e6])) * float(rng.choice([0.97, 0.995, 0.9995, 1.0, 1.0005, 1.005, 1.03]))
    n_near = int(rng.choice([3, 8, 40, 300, 1200]))
    a = np.sort(rng.uniform(0, 0.5 * np.pi, n_near))
    r = rng.uniform(8, 30) * (1 + 0.3 * rng.uniform(-1, 1, n_near))
    near = np.stack([20 + r * np.cos(a), 20 + r * np.sin(a)], 1)
    # the far part: a few vertices out at `far` (relative to the window's middle, the filter's origin), on either axis or both
    k = int(rng.integers(1, 4))
    sgn = rng.choice([-1.0, 1.0], 2)
    farp = np.stack([20 + sgn[0] * far * rng.uniform(0.2, 1.0, k), 20 + sgn[1] * far * rng.uniform(0.2, 1.0, k)], 1)
    farp[int(rng.integers(0, k)), int(rng.integers(0, 2))] = 20 + float(rng.choice([-1.0, 1.0])) * far   # one coordinate AT the bound
    pts = np.concatenate([near, farp])
    if rng.random() < 0.5:
        pts = np.round(pts * 64) / 64
    segs = ring(pts)
    if rng.random() < 0.5:  # the far vertices in a chunk of their own: duplicate the near part up to a chunk boundary
        pad = ring(near[::-1] * 0.5 + 10)
        segs = np.concatenate([pad, segs])
    w = int(rng.integers(30, 60))
    return segs, 0, 0, w, w


def fuzz_boundary():
    rng = np.random.default_rng(20)
    return MarginSet("fuzz_boundary", [boundary_glyph(rng) for _ in range(32)])


def fuzz_guards():
    rng = np.random.default_rng(21)
    return MarginSet("fuzz_guards", [guard_glyph(rng) for _ in range(32)], M=4096)


# ---------------------------------------------------------------------------------------------------------------
# the sets the suite had before (tests/test_gpu_kernel_edge.py), for the instances of the margins build
# ---------------------------------------------------------------------------------------------------------------
def old_sets():
    """every glyph-list input set of tests/test_gpu_kernel_edge.py, from its own generator (the remaining tests there render
    the synthetic outline batch, or check arguments, threads and variant ids: no raster inputs of their own)"""
    import test_gpu_kernel_edge as E
    gens = {"random_small": E.glyphs_random_small, "random_multichunk": E.glyphs_random_multichunk,
            "overlapping_rings": E.glyphs_overlapping_rings, "on_vertices_and_rows": E.glyphs_on_vertices_and_rows,
            "many_ties": E.glyphs_many_ties, "on_boundaries": E.glyphs_on_rounding_boundaries,
            "finely_flattened": E.glyphs_finely_flattened, "tall_localised_chunks": E.glyphs_tall_localised_chunks,
            "wide_and_thin": E.glyphs_wide_and_thin, "big_far": E.glyphs_big_and_far, "tiny": E.glyphs_tiny}
    return [MarginSet("old_" + name, gen()) for name, gen in gens.items()]


NEW_SETS = (
    near_boundary, near_subulp,
    lambda: near_M("1e3", 1000), lambda: near_M("4000", 4000), lambda: near_M("4200", 4200),
    lambda: near_M("1e6lo", 990000), lambda: near_M("1e6hi", 1010000),
    abs_position,
    lambda: lanes(1), lambda: lanes(2), lambda: lanes(3), lanes_row,
    argmin_swap, cand_long_in_group, cand_equality, cand_sat_far, box_reach, box_band, guard_huge,
    fuzz_boundary, fuzz_guards,
)


@lru_cache(maxsize=None)
def new_sets():
    """name -> MarginSet, every set built once per process"""
    sets = [f() for f in NEW_SETS]
    return {s.name: s for s in sets}
