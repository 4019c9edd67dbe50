"""Rule U restated in plain f64 arithmetic, and the sets the union tests share.

`union_segments` follows csrc/outline_union_pass.inc operation for operation: every product, difference and quotient below
is one IEEE f64 operation (numpy's element-wise ufuncs never fuse), taken in the order the device takes it, so the device's
pieces can be compared bit for bit.  The limit mirrors csrc/outline_union_limits.h.

The yardstick (`rect_union_boundary`) shares no code with the restatement: it fills the grid of all coordinates of a
rectilinear set from the signed rectangles themselves and takes the edges between filled and empty cells.
"""
from __future__ import annotations

import struct

import numpy as np

UNION_MAX_SEGMENTS = 6144  # VGSDF_UNION_MAX_SEGMENTS
STATE_IDENTITY, STATE_REBUILT, STATE_OVER_LIMIT, STATE_NON_FINITE = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ the restatement
class _Glyph:
    """A glyph's segments and what every pair computation needs of them.  The pair functions take a block of segments `ks`
    (rows) against all partners (columns)."""

    def __init__(self, segs):
        s = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4)
        self.n = len(s)
        self.sx, self.sy, self.ex, self.ey = (s[:, i].copy() for i in range(4))
        self.dx = self.ex - self.sx
        self.dy = self.ey - self.sy
        self.live = ~((self.sx == self.ex) & (self.sy == self.ey))  # zero-length segments take no part
        self.idx = np.arange(self.n)

    def pair(self, ks):
        """-> (crossing, coincident, parameter on k, shared point x, y), each [len(ks), n].  Every pair is computed from its
        member of lower index i (r = s_j - s_i, t along i, u along j) whichever of the two asks."""
        ks = np.asarray(ks)
        lo = self.idx[None, :] < ks[:, None]  # the partner is i, k is j

        def ij(a):
            return np.where(lo, a[None, :], a[ks][:, None]), np.where(lo, a[ks][:, None], a[None, :])
        (ix, jx), (iy, jy), (iex, jex), (iey, jey) = ij(self.sx), ij(self.sy), ij(self.ex), ij(self.ey)
        (dix, djx), (diy, djy) = ij(self.dx), ij(self.dy)
        rx = jx - ix
        ry = jy - iy
        den = dix * djy - diy * djx
        ct = rx * djy - ry * djx
        cu = rx * diy - ry * dix
        with np.errstate(all="ignore"):
            t = ct / den
            u = cu / den
            px = ix + t * dix
            py = iy + t * diy
        ok = self.live[None, :] & (self.idx[None, :] != ks[:, None]) & self.live[ks][:, None]
        cross = ok & (den != 0.0) & (t >= 0.0) & (t <= 1.0) & (u >= 0.0) & (u <= 1.0)
        coinc = ok & (den == 0.0) & (cu == 0.0)
        # the shared point (U2): an end point as it stands where a parameter is exactly 0 or 1 (t before u, 0 before 1),
        # else the point computed from segment i
        for cond, qx, qy in ((u == 1.0, jex, jey), (u == 0.0, jx, jy), (t == 1.0, iex, iey), (t == 0.0, ix, iy)):
            px = np.where(cond, qx, px)
            py = np.where(cond, qy, py)
        return cross, coinc, np.where(lo, u, t), px, py

    def along(self, k, qx, qy):
        """parameter of the points q on segment k, by k's dominant axis"""
        with np.errstate(all="ignore"):
            if abs(self.dx[k]) >= abs(self.dy[k]):
                return (qx - self.sx[k]) / self.dx[k]
            return (qy - self.sy[k]) / self.dy[k]

    def cut_params(self, k, row):
        """the three candidate cuts per partner of segment k: (parameter on k or inf, x, y) of the crossing, of a coincident
        partner's start and of its end"""
        cross, coinc, tk, px, py = row
        return ((np.where(cross, tk, np.inf), px, py),
                (np.where(coinc, self.along(k, self.sx, self.sy), np.inf), self.sx, self.sy),
                (np.where(coinc, self.along(k, self.ex, self.ey), np.inf), self.ex, self.ey))


def _next_cut(cands, cur_t):
    """the lowest cut parameter above cur_t and its point; the partner of lowest index wins a tie, and of one partner the
    crossing before a coincident start before a coincident end.  None: no cut is left."""
    best = None
    for ct, cx, cy in cands:
        m = (ct > cur_t) & (ct < 1.0)
        if not m.any():
            continue
        tt = np.where(m, ct, np.inf)
        p = int(np.argmin(tt))  # first of the minima: lowest partner index
        c = (float(tt[p]), p, float(cx[p]), float(cy[p]))
        if best is None or c[0] < best[0] or (c[0] == best[0] and c[1] < best[1]):
            best = c
    return best


def _keep(g, ks, ax, ay, bx, by, coinc):
    """classify the pieces (a, b) of the segments ks at their midpoints against the original segments (rule U, step 4);
    all arguments by rows"""
    ks = np.asarray(ks)
    mx = (ax + bx) * 0.5
    my = (ay + by) * 0.5
    steep = np.abs(g.dy[ks]) >= np.abs(g.dx[ks])  # else: the same rule with x and y exchanged
    st = steep[:, None]
    SX, SY = np.where(st, g.sx[None, :], g.sy[None, :]), np.where(st, g.sy[None, :], g.sx[None, :])
    EX, EY = np.where(st, g.ex[None, :], g.ey[None, :]), np.where(st, g.ey[None, :], g.ex[None, :])
    mx, my = np.where(steep, mx, my)[:, None], np.where(steep, my, mx)[:, None]
    sg = np.where(np.where(steep, g.dy[ks], g.dx[ks]) > 0.0, 1, -1)
    up = (SY <= my) & (EY > my)
    down = (SY > my) & (EY <= my)
    other = g.live[None, :] & (g.idx[None, :] != ks[:, None])
    sign = np.where(other, up.astype(np.int64) - down.astype(np.int64), 0)
    grp = coinc & (sign != 0)
    step = sg + np.where(grp, sign, 0).sum(axis=1)
    lower_same = (grp & (g.idx[None, :] < ks[:, None]) & (sign == sg[:, None])).any(axis=1)
    with np.errstate(all="ignore"):
        t = (my - SY) / (EY - SY)
        x = SX + t * (EX - SX)
    w = np.where((sign != 0) & ~coinc & (x > mx), sign, 0).sum(axis=1)
    return ((w == 0) != (w + step == 0)) & ((step > 0) == (sg > 0)) & ~lower_same


def union_segments(segs, limit: int = UNION_MAX_SEGMENTS):
    """-> (pieces [m,4] f64, state).  Pieces in the order of their source segments, then along the segment."""
    s = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4)
    if len(s) > limit:
        return s.copy(), STATE_OVER_LIMIT
    if not np.isfinite(s).all():
        return s.copy(), STATE_NON_FINITE
    g = _Glyph(s)
    out = []
    changed = False
    rows = max(1, 400000 // max(g.n, 1))
    for k0 in range(0, g.n, rows):
        ks = np.arange(k0, min(k0 + rows, g.n))
        pairs = g.pair(ks)
        cross, coinc, tk = pairs[0], pairs[1], pairs[2]
        whole = _keep(g, ks, g.sx[ks], g.sy[ks], g.ex[ks], g.ey[ks], coinc)  # the segments as single pieces
        maybe_cut = (cross & (tk > 0.0) & (tk < 1.0)).any(axis=1) | coinc.any(axis=1)  # (the rows worth a closer look)
        for r, k in enumerate(ks):
            if not g.live[k]:
                continue
            cands = g.cut_params(k, [a[r] for a in pairs]) if maybe_cut[r] else ()
            if not any(((ct > 0.0) & (ct < 1.0)).any() for ct, _, _ in cands):
                if whole[r]:
                    out.append(tuple(s[k]))
                else:
                    changed = True
                continue
            changed = True
            cur_t, cx, cy = 0.0, float(g.sx[k]), float(g.sy[k])
            for _ in range(2 * g.n + 2):
                nxt = _next_cut(cands, cur_t)
                nx, ny = (float(g.ex[k]), float(g.ey[k])) if nxt is None else (nxt[2], nxt[3])
                if not (cx == nx and cy == ny):
                    one = np.array([k])
                    if _keep(g, one, np.array([cx]), np.array([cy]), np.array([nx]), np.array([ny]), coinc[r:r + 1])[0]:
                        out.append((cx, cy, nx, ny))
                if nxt is None:
                    break
                cur_t, cx, cy = nxt[0], nx, ny
    return np.array(out, dtype=np.float64).reshape(-1, 4), (STATE_REBUILT if changed else STATE_IDENTITY)


# ------------------------------------------------------------------------------------------------ the properties
def winding_nonzero(segs, x0, y0, w, h):
    """wn != 0 at every pixel centre of the rect by the reference's crossing rule -> bool [h, w] (row 0 = y0)"""
    s = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((h, w), dtype=bool)
    px = np.arange(w) + (x0 + 0.5)
    for r in range(h):
        py = r + (y0 + 0.5)
        up = (s[:, 1] <= py) & (s[:, 3] > py)
        dn = (s[:, 1] > py) & (s[:, 3] <= py)
        m = up | dn
        if not m.any():
            continue
        q = s[m]
        sign = np.where(up[m], 1, -1)
        t = (py - q[:, 1]) / (q[:, 3] - q[:, 1])
        x = q[:, 0] + t * (q[:, 2] - q[:, 0])
        wn = -((x[None, :] <= px[:, None]) * sign[None, :]).sum(axis=1)
        out[r] = wn != 0
    return out


def open_points(pieces):
    """points (as f64 bit patterns) where the pieces that start there and those that end there differ in number (U2)"""
    bal = {}
    for ax, ay, bx, by in np.asarray(pieces, dtype=np.float64).reshape(-1, 4):
        a, b = struct.pack("<dd", ax, ay), struct.pack("<dd", bx, by)
        bal[a] = bal.get(a, 0) + 1
        bal[b] = bal.get(b, 0) - 1
    return [struct.unpack("<dd", k) for k, v in bal.items() if v]


def rect_of(segs, pad: int = 3):
    s = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    x0 = int(np.floor(min(s[:, 0].min(), s[:, 2].min()))) - pad
    y0 = int(np.floor(min(s[:, 1].min(), s[:, 3].min()))) - pad
    x1 = int(np.ceil(max(s[:, 0].max(), s[:, 2].max()))) + pad
    y1 = int(np.ceil(max(s[:, 1].max(), s[:, 3].max()))) + pad
    return x0, y0, x1 - x0, y1 - y0


# ------------------------------------------------------------------------------------------------ the exact sets
def ring(pts):
    p = [(float(x), float(y)) for x, y in pts]
    return [(p[i][0], p[i][1], p[(i + 1) % len(p)][0], p[(i + 1) % len(p)][1]) for i in range(len(p))]


def rect(x0, y0, x1, y1, sign=+1):
    """sign +1: counter-clockwise (wn +1 inside), -1: clockwise"""
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return ring(pts if sign > 0 else pts[::-1])


def _comb(teeth):
    # the bar is 512 long so that the teeth cut its long edges at parameters c / 512: exact
    bar = [(0.0, 4.0, 512.0, 7.0, +1)]
    return bar + [(1.0 + 7.0 * i, 1.0, 4.0 + 7.0 * i, 10.0, +1) for i in range(teeth)]


# rectilinear sets as signed rectangles (x0, y0, x1, y1, sign): the yardstick reads the same records
RECT_SETS = {
    "two_rects": [(4, 4, 20, 10, +1), (8, 6, 12, 22, +1)],
    "plus": [(2, 8, 22, 14, +1), (9, 1, 15, 21, +1)],
    "tee": [(2, 16, 22, 21, +1), (9.5, 2, 14.5, 16, +1), (9.5, 15, 14.5, 18, +1)],
    "abut_whole_edge": [(2, 2, 10, 12, +1), (10, 2, 19, 12, +1)],
    "abut_part_edge": [(2, 2, 10, 12, +1), (10, 5, 19, 9, +1)],
    "duplicate": [(3, 3, 15, 11, +1), (3, 3, 15, 11, +1)],
    "reverse_cancels": [(3, 3, 15, 11, +1), (3, 3, 15, 11, -1)],
    "hole": [(2, 2, 22, 22, +1), (8, 8, 16, 16, -1)],
    "nested_same": [(2, 2, 22, 22, +1), (8, 8, 16, 16, +1)],
    "counter_overlap": [(2, 2, 14, 14, +1), (8, 8, 20, 20, -1)],
    "corner_touch": [(2, 2, 10, 10, +1), (10, 10, 18, 18, +1)],
    "comb70": _comb(70),
}


def rect_set_segments(name):
    return np.array([s for r in RECT_SETS[name] for s in rect(*r)], dtype=np.float64)


def _diamond(cx, cy, r):
    return ring([(cx + r, cy), (cx, cy + r), (cx - r, cy), (cx, cy - r)])


# sets with oblique edges: (input, expected boundary pieces as an undirected point set, see `as_point_set`)
def _oblique_sets():
    sets = {}
    # two 45-degree diamonds crossing at even coordinates: centres (10, 10) and (16, 10), radius 6; they cross at (13, 7), (13, 13)
    a, b = _diamond(10, 10, 6), _diamond(16, 10, 6)
    want = ring([(13, 7), (16, 4), (22, 10), (16, 16), (13, 13), (10, 16), (4, 10), (10, 4)])
    sets["diamonds"] = (np.array(a + b), np.array(want))
    # figure eight: one contour through (10, 10) twice; the lobes wind +1 and -1, all of it is boundary
    eight = ring([(2, 2), (18, 18), (18, 2), (2, 18)])
    sets["figure_eight"] = (np.array(eight), np.array(eight))
    # a vertex of the triangle lies on the square's right edge, and both of its neighbours cut that edge there
    sq = rect(2, 2, 12, 22)
    tri = ring([(12, 12), (20, 4), (20, 20)])
    sets["vertex_on_edge"] = (np.array(sq + tri), np.array(sq + tri))
    # the same with the triangle's vertex pushed through: the tip lies inside the square
    tri2 = ring([(8, 12), (20, 0), (20, 24)])
    want2 = ring([(2, 2), (12, 2), (12, 8), (20, 0), (20, 24), (12, 16), (12, 22), (2, 22)])
    sets["tip_inside"] = (np.array(sq + tri2), np.array(want2))
    return sets


OBLIQUE_SETS = _oblique_sets()


def exact_sets():
    """name -> segments [n,4] of every exact set"""
    d = {k: rect_set_segments(k) for k in RECT_SETS}
    d.update({k: v[0] for k, v in OBLIQUE_SETS.items()})
    return d


# ------------------------------------------------------------------------------------------------ the yardstick
def rect_union_boundary(rects):
    """Boundary of { wn != 0 } of signed rectangles, as unit edges of the grid of all their coordinates: directed so that a
    filled cell of positive winding lies on the left, one of negative winding on the right.  -> [m,4]"""
    xs = sorted({float(v) for r in rects for v in (r[0], r[2])})
    ys = sorted({float(v) for r in rects for v in (r[1], r[3])})
    wn = np.zeros((len(ys) + 1, len(xs) + 1), dtype=np.int64)  # cell (r, c) = [ys[r-1], ys[r]] x [xs[c-1], xs[c]]; a rim of empty cells
    for x0, y0, x1, y1, sign in rects:
        c0, c1, r0, r1 = xs.index(float(x0)), xs.index(float(x1)), ys.index(float(y0)), ys.index(float(y1))
        wn[r0 + 1:r1 + 1, c0 + 1:c1 + 1] += sign
    out = []
    for r in range(len(ys)):  # horizontal edges on y = ys[r]: below is cell row r, above row r + 1
        for c in range(1, len(xs)):
            lo, hi = wn[r, c], wn[r + 1, c]
            if (lo != 0) == (hi != 0):
                continue
            a, b = (xs[c - 1], ys[r]), (xs[c], ys[r])  # left to right: above is on the left
            fwd = (hi > 0) if hi != 0 else (lo < 0)
            out.append(a + b if fwd else b + a)
    for c in range(len(xs)):  # vertical edges on x = xs[c]: left is cell column c, right column c + 1
        for r in range(1, len(ys)):
            le, ri = wn[r, c], wn[r, c + 1]
            if (le != 0) == (ri != 0):
                continue
            a, b = (xs[c], ys[r - 1]), (xs[c], ys[r])  # upwards: the left cell is on the left
            fwd = (le > 0) if le != 0 else (ri < 0)
            out.append(a + b if fwd else b + a)
    return np.array(out, dtype=np.float64).reshape(-1, 4)


def as_point_set(pieces):
    """Pieces as a point set that can be compared: per supporting line (in exact rational form for the integer and
    half-integer coordinates of the exact sets) the merged intervals the pieces cover."""
    from fractions import Fraction as F
    lines = {}
    for ax, ay, bx, by in np.asarray(pieces, dtype=np.float64).reshape(-1, 4):
        ax, ay, bx, by = F(ax), F(ay), F(bx), F(by)
        dx, dy = bx - ax, by - ay
        if dx == 0 and dy == 0:
            continue
        if dx < 0 or (dx == 0 and dy < 0):
            dx, dy = -dx, -dy
        n = max(abs(dx), abs(dy))
        dx, dy = dx / n, dy / n  # one direction per line
        c = ax * dy - ay * dx  # which of the parallels
        pa, pb = sorted((ax * dx + ay * dy, bx * dx + by * dy))
        lines.setdefault((dx, dy, c), []).append((pa, pb))
    out = set()
    for key, iv in lines.items():
        iv.sort()
        cur = list(iv[0])
        for a, b in iv[1:]:
            if a <= cur[1]:
                cur[1] = max(cur[1], b)
            else:
                out.add((key, tuple(cur)))
                cur = [a, b]
        out.add((key, tuple(cur)))
    return out


# ------------------------------------------------------------------------------------------------ wave and chunk edges
def polygon(n, cx=40.0, cy=40.0, r=30.0, sign=+1):
    """a convex ring of n segments on a circle (identity under rule U)"""
    a = np.arange(n) * (2.0 * np.pi / n) * sign
    return np.array(ring(list(zip(cx + r * np.cos(a), cy + r * np.sin(a)))))


def sized_glyph(n):
    """n segments that rule U rebuilds: a polygon of n - 4 segments and a rectangle across it"""
    return np.concatenate([polygon(n - 4), np.array(rect(5, 35, 75, 45))])


def unlike_neighbours(n_glyphs):
    """glyph i of the batch: identity, rebuilt, cancelled, empty by i % 4"""
    kinds = [polygon(7, 20.0, 20.0, 15.0), rect_set_segments("two_rects"), rect_set_segments("reverse_cancels"), np.zeros((0, 4))]
    return [kinds[i % 4] for i in range(n_glyphs)]


def with_rects(glyphs):
    """[(segs, x0, y0, w, h)] of segment arrays, the form of make_batch: the bounding box and 3 px on every side; a glyph
    without segments gets 8 x 8 px, one with a coordinate that is not finite no pixels (its raster is not this suite's)"""
    out = []
    for g in glyphs:
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(-1, 4)
        out.append((g,) + ((0, 0, 0, 0) if not np.isfinite(g).all() else rect_of(g) if len(g) else (0, 0, 8, 8)))
    return out


def union_glyphs(glyphs, limit: int = UNION_MAX_SEGMENTS):
    """rule U restated over [(segs, x0, y0, w, h)] -> (the same with the pieces for segments, states u8[n])"""
    res = [union_segments(g[0], limit) for g in glyphs]
    return [(r[0],) + tuple(g[1:]) for r, g in zip(res, glyphs)], np.array([r[1] for r in res], dtype=np.uint8)


def rings_of(segs):
    """the contours of a segment list as point arrays (a contour ends where a segment does not start at its predecessor's end)"""
    s = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    rings, cur = [], []
    for i, (sx, sy, ex, ey) in enumerate(s):
        if cur and not (s[i - 1, 2] == sx and s[i - 1, 3] == sy):
            rings.append(np.array(cur))
            cur = []
        cur.append((sx, sy))
    if cur:
        rings.append(np.array(cur))
    return rings


# ------------------------------------------------------------------------------------------------ fixture glyphs
NAMED_NOTO = (0x00C5, 0x00C7, 0x0104, 0x0224)
# the glyphs among the first 600 code points of Noto Sans Regular that rule U rebuilds (tests/test_union_outline_host.py holds the
# list against the restatement)
REBUILT_NOTO = (0x00C5, 0x00C7, 0x00E7, 0x0104, 0x0105, 0x0118, 0x0119, 0x012E, 0x012F, 0x015E, 0x015F, 0x0162, 0x0163, 0x0167, 0x0172,
                0x0173, 0x01EA, 0x01EB, 0x01EC, 0x01ED, 0x0224, 0x0228, 0x0229, 0x023A, 0x023B, 0x023C, 0x023D, 0x023E, 0x0244, 0x0246,
                0x0247, 0x024C, 0x024D, 0x024E, 0x024F, 0x025D, 0x0268, 0x0289)


def font_glyphs(path, n_code_points=600):
    """[(code point, info, segs)] of the glyphs with a bitmap among the first n_code_points of the face's cmap"""
    from oracle import oracle as O
    f = O.Font(path)
    out = []
    for cp in f.codepoints()[:n_code_points]:
        r = f.prepare_glyph(int(cp))
        if r is not None and r[0].has_bitmap:
            out.append((int(cp), r[0], r[1]))
    return out
