"""The flattening passes of the device front-end (outline_count / outline_emit_segments, csrc/outline_kernels.hip) restated
on the CPU, and the command streams that drive them into each of their branches.  test_gpu_flatten_regimes.py runs the
streams on the GPU; this module proves, without one, that every stream lands where it was written for.

Restated in f64 on the f32 command coordinates (the current point is the previous command's (x, y)):

  quad_split      the depth L of a quadratic's complete tree, or None: the sequential walk
  cubic_bound     the depth bound D of a cubic's adaptive tree (D <= 6), or None: the sequential walk
  cubic_leaves    the reference's own subdivision (ring.rs:159-187): every leaf's depth and its first candidate
  items_of_depth  the items a command of 2^depth points / candidates hands to the parallel rounds

Families (each a list of glyphs; a family starts on a wave boundary of the batch):

  A  cubic depth-bound edge     M = sqrt(16^D / 808) (1 +- 1e-3), (1 +- 0.02), D = 0..6, in D1 / D2, x / y, both signs
  B  cubic tree shapes          collinear (a flat root over 2^(D-3) items), a = s and b = e, four equal points, control
                                points bunched at either end, S-curves, loops, cusps; every leaf depth 0..6
  C  coordinate bounds          max |coordinate| = 1e6 and 1e6 + 0.0625 in every position (the current point included),
                                parallel quadratics of L = 9..13, quadratics on both sides of the uncapped walk's bounds
  D  deep sequential cubics     bounds 7..16 alone in their wave; 64 cubics of bound 7..12 in one wave
  E  wave composition           an item owner at lane 0 behind lane 63, glyphs from lanes 0 / 1 / 63, commands without
                                items between owners (at lane 63 too), wave item totals 64 / 65 / 128 / 129 / 1000+,
                                parallel and sequential commands side by side
  F  ring state across steps    200 cubics without a state change, close / line at glyph command 63, glyphs of 1024 and
                                1025 commands
  G  non-monotone transforms    A, B and E at scales -24/1000 and -1/32 (every command walks sequentially)

Also here, CPU only: a CFF font whose charstrings carry families A, B, D and F, through the host's flattening
(FontManager.build_batch) and the dummy raster, against the oracle."""
import math
from collections import Counter

import numpy as np
import pytest

M, L, Q, C3, Z = 0, 1, 2, 3, 4
TOL = 0.01            # ring_builder.rs:62 precision, passed as tolerance_sq
ITEM_DEPTH = 3        # an item = a subtree of up to 2^3 leaves
MAX_PAR_DEPTH = 6     # cubics with a deeper bound walk sequentially
BIG = 1.0e6           # coordinate bound of both parallel forms
NEXT = float(np.nextafter(np.float32(BIG), np.float32(np.inf)))   # 1e6 + 0.0625
UNIT = 24.0 / 1000.0


def f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------
# the split rules, restated
# ---------------------------------------------------------------------------------------------------------------------

def quad_split(s, c, e):
    """quad_parallel_points: the depth L of the complete tree, or None (sequential walk)"""
    dx = s[0] + e[0] - c[0] * 2.0
    dy = s[1] + e[1] - c[1] * 2.0
    D = dx * dx + dy * dy
    m = max(abs(s[0]), abs(s[1]), abs(c[0]), abs(c[1]), abs(e[0]), abs(e[1]))
    if not (D <= 7.2e14 and m <= BIG):
        return None
    v, lev = D, 0
    while v > TOL:
        v *= 0.0625
        lev += 1
    if v <= TOL * (1.0 - 1.0e-6) and (lev == 0 or v * 16.0 > TOL * (1.0 + 1.0e-6)):
        return lev
    return None


def quad_walk_capped(s, c, e):
    """flatten_quad_any: True when the sequential walk is the capped one"""
    dx = s[0] + e[0] - c[0] * 2.0
    dy = s[1] + e[1] - c[1] * 2.0
    m = max(abs(s[0]), abs(s[1]), abs(c[0]), abs(c[1]), abs(e[0]), abs(e[1]))
    return not (dx * dx + dy * dy <= 7.2e14 and m <= 1.0e9)


def cubic_need(s, a, b, e):
    """the first level D with 16^D >= 1.01 * 800 * M^2 (no cap), and m"""
    d1x, d1y = s[0] - 2.0 * a[0] + b[0], s[1] - 2.0 * a[1] + b[1]
    d2x, d2y = a[0] - 2.0 * b[0] + e[0], a[1] - 2.0 * b[1] + e[1]
    Mx = max(abs(d1x), abs(d1y), abs(d2x), abs(d2y))
    m = max(abs(v) for p in (s, a, b, e) for v in p)
    need = 1.01 * 800.0 * Mx * Mx
    v, D = 1.0, 0
    while v < need:
        v *= 16.0
        D += 1
    return D, Mx, m


def cubic_bound(s, a, b, e):
    """cubic_parallel_depth: the depth bound D <= 6, or None (sequential walk)"""
    D, Mx, m = cubic_need(s, a, b, e)
    if not (Mx <= BIG and m <= BIG) or D > MAX_PAR_DEPTH:
        return None
    return D


def items_of_depth(depth):
    return 1 << (depth - ITEM_DEPTH) if depth > ITEM_DEPTH else 1


def _cubic_flat(n):
    dx = (n[4] + n[2]) - (n[0] + n[6])
    dy = (n[5] + n[3]) - (n[1] + n[7])
    return dx * dx + dy * dy <= TOL


def _cubic_split(n):
    s0, s1, a0, a1, b0, b1, e0, e1 = n
    p01x, p01y = (s0 + a0) / 2.0, (s1 + a1) / 2.0
    p12x, p12y = (a0 + b0) / 2.0, (a1 + b1) / 2.0
    p23x, p23y = (b0 + e0) / 2.0, (b1 + e1) / 2.0
    p012x, p012y = (p01x + p12x) / 2.0, (p01y + p12y) / 2.0
    p123x, p123y = (p12x + p23x) / 2.0, (p12y + p23y) / 2.0
    mx, my = (p012x + p123x) / 2.0, (p012y + p123y) / 2.0
    return (s0, s1, p01x, p01y, p012x, p012y, mx, my), (mx, my, p123x, p123y, p23x, p23y, e0, e1)


_LEAVES = {}


def cubic_leaves(s, a, b, e):
    """ring.rs:159-187 (the reference's stack walk, left half first): [(depth, path bits, end x, end y)] in order"""
    key = (s, a, b, e)
    if key not in _LEAVES:
        out = []
        stack = [((s[0], s[1], a[0], a[1], b[0], b[1], e[0], e[1]), 0, 0)]
        while stack:
            n, d, p = stack.pop()
            if _cubic_flat(n):
                out.append((d, p, n[6], n[7]))
                continue
            lo, hi = _cubic_split(n)
            stack.append((hi, d + 1, 2 * p + 1))
            stack.append((lo, d + 1, 2 * p))
        _LEAVES[key] = out
    return _LEAVES[key]


def first_candidates(leaves, D):
    """each leaf's first candidate among the 2^D of the complete tree of depth D"""
    return [p << (D - d) for d, p, _, _ in leaves]


def quad_points(s, c, e):
    """ring.rs:119-144: how many points a quadratic appends"""
    n, stack = 0, [(s, c, e)]
    while stack:
        s_, c_, e_ = stack.pop()
        dx = s_[0] + e_[0] - c_[0] * 2.0
        dy = s_[1] + e_[1] - c_[1] * 2.0
        if dx * dx + dy * dy <= TOL:
            n += 1
            continue
        m1 = ((s_[0] + c_[0]) / 2.0, (s_[1] + c_[1]) / 2.0)
        m2 = ((c_[0] + e_[0]) / 2.0, (c_[1] + e_[1]) / 2.0)
        mid = ((m1[0] + m2[0]) / 2.0, (m1[1] + m2[1]) / 2.0)
        stack.append((mid, m2, e_))
        stack.append((s_, m1, mid))
    return n


# ---------------------------------------------------------------------------------------------------------------------
# per command: ring state, class, items, points (what outline_context / outline_count decide)
# ---------------------------------------------------------------------------------------------------------------------

def command_classes(stream, monotone=True):
    """[(cls, items, points, info)] per command of one glyph.  cls: move, line, close, ignored (curve on an empty ring),
    quad-par, quad-seq, quad-capped, cubic-par, cubic-seq; monotone=False: every command that appends points walks."""
    out, open_, cur = [], False, None
    for k, x1, y1, x2, y2, x, y in stream:
        e = (float(x), float(y))
        if k in (M, L):
            out.append(("move" if k == M else "line", 1 if monotone else 0, 1, None))
            open_, cur = True, e
        elif k == Z:
            out.append(("close", 0, 0, None))
            open_ = False
        elif not open_:
            out.append(("ignored", 0, 0, None))
        elif k == Q:
            c = (float(x1), float(y1))
            lev = quad_split(cur, c, e)
            if lev is not None and monotone:
                out.append(("quad-par", items_of_depth(lev), 1 << lev, lev))
            else:
                cls = "quad-capped" if quad_walk_capped(cur, c, e) else "quad-seq"
                out.append((cls, 0, 1 << lev if lev is not None else quad_points(cur, c, e), lev))
            cur = e
        else:
            a, b = (float(x1), float(y1)), (float(x2), float(y2))
            D = cubic_bound(cur, a, b, e)
            leaves = cubic_leaves(cur, a, b, e)
            if D is not None and monotone:
                out.append(("cubic-par", items_of_depth(D), len(leaves), (D, leaves)))
            else:
                out.append(("cubic-seq", 0, len(leaves), (cubic_need(cur, a, b, e)[0], leaves)))
            cur = e
    return out


def ring_lengths(stream, classes=None):
    """RingBuilder (ring_builder.rs:26-117, ring.rs:53-63) on the restated point counts: the point count of every saved
    ring, the appended copy of point 0 included"""
    classes = classes or command_classes(stream)
    rings, n, first, last = [], 0, None, None

    def save():
        if n >= 3:
            app = abs(first[0] - last[0]) > 2.220446049250313e-16 or abs(first[1] - last[1]) > 2.220446049250313e-16
            if n + app >= 4:
                rings.append(n + app)

    for cmd, (cls, _, pts, _) in zip(stream, classes):
        p = (float(cmd[5]), float(cmd[6]))
        if cls == "move":
            save()
            n, first, last = 1, p, p
        elif cls == "line":
            if n == 0:
                first = p
            n, last = n + 1, p
        elif cls == "close":
            save()
            n = 0
        elif cls != "ignored":
            n, last = n + pts, p
    save()
    return rings


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------

class Glyph:
    def __init__(self, name, stream, scale=UNIT, shift=0.0, tags=()):
        self.name = name
        self.stream = [(int(c[0]),) + tuple(f32(v) for v in c[1:]) for c in stream]
        self.scale, self.shift = float(scale), float(shift)
        self.tags = set(tags)


def _mv(p):
    return (M, 0, 0, 0, 0, p[0], p[1])


def _ln(p):
    return (L, 0, 0, 0, 0, p[0], p[1])


def _cu(a, b, e):
    return (C3, a[0], a[1], b[0], b[1], e[0], e[1])


def _qu(c, e):
    return (Q, c[0], c[1], 0, 0, e[0], e[1])


_CL = (Z, 0, 0, 0, 0, 0, 0)


def _shift_of(i):
    return ((i * 37) % 64 - 32) / 128.0


def family_a():
    """the depth bound's edge: M just inside and outside sqrt(16^D / 808).  Every coordinate is a multiple of
    q = 2^-13 of M's binade and below 2^24 q: exact in f32, and so is M, which carries 14 significant bits"""
    out = []
    for D in range(7):
        m0 = math.sqrt(16.0 ** D / 808.0)
        q = 2.0 ** (math.floor(math.log2(m0)) - 13)
        r = lambda v: round(v / q) * q  # noqa: E731
        for f in (1 - 1e-3, 1 + 1e-3, 1 - 0.02, 1 + 0.02):
            for which in (1, 2):
                for axis in (0, 1):
                    for sign in (1, -1):
                        big = r(sign * m0 * f)
                        d_main = [0.0, 0.0]
                        d_main[axis] = big
                        d_main[1 - axis] = r(0.37 * m0)
                        d_other = (r(-0.21 * m0), r(0.13 * m0))
                        d1, d2 = (d_main, d_other) if which == 1 else (d_other, d_main)
                        s = (r(40 * m0), r(-24 * m0))
                        u = (r(16 * m0), r(5 * m0))
                        a = (s[0] + u[0], s[1] + u[1])
                        b = (s[0] + 2 * u[0] + d1[0], s[1] + 2 * u[1] + d1[1])
                        e = (-a[0] + 2 * b[0] + d2[0], -a[1] + 2 * b[1] + d2[1])
                        st = [_mv(s), _cu(a, b, e), _ln((s[0] + u[0], s[1] - r(20 * m0))), _CL]
                        out.append(Glyph(f"A:D{D}:f{f:g}:D{which}{'xy'[axis]}{sign:+d}", st, shift=_shift_of(len(out))))
    return out


def _b_shapes(k, o=(100.0, 200.0)):
    """(name, s, a, b, e) of size k"""
    ox, oy = o
    P = lambda x, y: (ox + x, oy + y)  # noqa: E731
    out = []
    for dname, (vx, vy) in (("h", (1, 0)), ("v", (0, 1)), ("d", (1, 1)), ("m", (-1, 0.5))):
        v = (k * vx, k * vy)
        out.append((f"collinear-{dname}", P(0, 0), P(0.75 * v[0], 0.75 * v[1]), P(0.25 * v[0], 0.25 * v[1]), P(*v)))
        for bend in (0.06, 0.2, 0.5, 1.5):   # a bend across the line: flat a level or two below the root
            w = (-vy * bend, vx * bend)
            out.append((f"bent{bend}-{dname}", P(0, 0), P(0.75 * v[0] + w[0], 0.75 * v[1] + w[1]),
                        P(0.25 * v[0] + w[0], 0.25 * v[1] + w[1]), P(*v)))
    out.append(("uniform-line", P(0, 0), P(k / 3, k / 6), P(2 * k / 3, k / 3), P(k, k / 2)))
    out.append(("a=s,b=e", P(0, 0), P(0, 0), P(k, 0.3 * k), P(k, 0.3 * k)))
    out.append(("bunched-start", P(0, 0), P(0.02 * k, 0.01 * k), P(0.05 * k, 0.3 * k), P(k, 0)))
    out.append(("bunched-end", P(0, 0), P(0.95 * k, 0.3 * k), P(0.98 * k, 0.01 * k), P(k, 0)))
    out.append(("s-curve", P(0, 0), P(k / 3, k / 2), P(2 * k / 3, -k / 2), P(k, 0)))
    out.append(("loop", P(0, 0), P(1.5 * k, k), P(-0.5 * k, k), P(k, 0)))
    out.append(("cusp", P(0, 0), P(k, k), P(0, k), P(k, 0)))
    return out


def family_b():
    out = []
    p = (300.0, 300.0)
    out.append(Glyph("B:four-equal", [_mv(p), _cu(p, p, p), _ln((p[0] + 50, p[1] - 40)), _CL], shift=0.25))
    for j in range(-6, 17):
        k = 2.0 ** (j / 2.0)
        for name, s, a, b, e in _b_shapes(k):
            s, a, b, e = [(f32(x), f32(y)) for x, y in (s, a, b, e)]
            if cubic_bound(s, a, b, e) is None:
                continue
            st = [_mv(s), _cu(a, b, e), _ln((s[0] + k / 2, s[1] - k - 5)), _CL]
            out.append(Glyph(f"B:{name}:k{k:g}", st, shift=_shift_of(len(out))))
    return out


def family_c():
    out = []
    B_ = BIG

    def cubic_base():
        return [(B_ - 20, B_ - 16), (B_ - 14, B_ - 2), (B_ - 6, B_ - 12), (B_ - 2, B_ - 18)]

    def quad_base():
        return [(B_ - 20, B_ - 16), (B_ - 10, B_ - 2), (B_ - 2, B_ - 18)]

    for kind in ("cubic", "quad"):
        for pos in range(8 if kind == "cubic" else 6):
            for val in (BIG, NEXT):
                for sign in (1, -1):
                    pts = cubic_base() if kind == "cubic" else quad_base()
                    pts = [list(p) for p in pts]
                    pts[pos // 2][pos % 2] = val
                    pts = [(sign * x, sign * y) for x, y in pts]
                    s = pts[0]
                    back = (sign * (B_ - 20), sign * (B_ - 20))
                    from_line = (pos // 2 + (sign < 0)) % 2 == 1   # the current point from a move / from a line
                    lead = [_mv(back), _ln(s)] if from_line else [_mv(s)]
                    curve = _cu(pts[1], pts[2], pts[3]) if kind == "cubic" else _qu(pts[1], pts[2])
                    st = lead + [curve, _ln((sign * (B_ - 19), sign * (B_ - 25)) if from_line else back), _CL]
                    out.append(Glyph(f"C:{kind}:pos{pos}:{val:.4f}:{sign:+d}", st, shift=_shift_of(len(out))))
    # parallel quadratics of L = 9..13 near the bound (at 2^-12 px per unit: the rect stays a few hundred px)
    for lev in range(9, 14):
        dev = round(0.1 * 4.0 ** lev * 0.55)
        w = min(dev, 1_900_000)
        s = (B_ - w, B_ - dev // 2 - 1000)
        e = (B_, s[1])
        c = ((s[0] + e[0]) / 2, s[1] + dev / 2)
        st = [_mv(s), _qu(c, e), _ln(((s[0] + e[0]) / 2, s[1] - 4096)), _CL]
        out.append(Glyph(f"C:quad-L{lev}", st, scale=2.0 ** -12, shift=0.125))
    # the sequential quadratic walks: uncapped (|d|^2 <= 7.2e14 and m <= 1e9) and capped, at m up to 1e9 (2^-16 px per unit)
    dev0 = math.sqrt(7.2e14)
    for name, rel, top in (("uncapped@1e9", -1e-4, 1.0e9), ("capped-D", 1e-4, 1.0e9 - 1.0e8), ("capped-m", -1e-4, 1.0e9 + 64),
                           ("uncapped@2e6", -1e-4, 3.0e7)):
        dev = round(dev0 * (1 + rel) / 128) * 128
        s = (top - 2 * dev, top - dev)
        e = (top - dev, top - dev)
        c = ((s[0] + e[0]) / 2, top - dev / 2)
        if name == "capped-m":
            s = (top, s[1])
            c = ((s[0] + e[0]) / 2 - 64, c[1])
        st = [_mv(s), _qu(c, e), _ln((s[0], s[1] - 65536)), _CL]
        out.append(Glyph(f"C:{name}", st, scale=2.0 ** -16, shift=-0.25))
    return out


def _s_curve(s, k, sign=1):
    """S-curve from s with second differences of 3k (M = 3k), chord (sign k, 0); (a + b) - (s + e) = 0: flat at the root"""
    return ((s[0] + sign * k / 3, s[1] + k), (s[0] + sign * 2 * k / 3, s[1] - k), (s[0] + sign * k, s[1]))


def _arch(s, k, sign=1):
    """an arch from s with M = k, chord (sign k, 0): (a + b) - (s + e) = (0, 2k), it keeps splitting to its bound"""
    return ((s[0], s[1] + k), (s[0] + sign * k, s[1] + k), (s[0] + sign * k, s[1]))


def deep_m(D, f=0.7):
    return f * math.sqrt(16.0 ** D / 808.0)


def family_d():
    """glyphs of 64 commands that start on a wave boundary: the deep cubic is the only sequential walk in its wave"""
    out = []
    for D in range(7, 17):
        k = deep_m(D)
        sc = 2.0 ** -round(math.log2(k / 200.0))
        s = (f32(k / 5), f32(k / 3))
        a, b, e = _arch(s, k)
        st = [_mv(s), _cu(a, b, e), _ln((s[0] + k / 2, s[1] - k / 2))] + [_CL] * 61
        out.append(Glyph(f"D:bound{D}", st, scale=sc, shift=0.375, tags={"align"}))
    # 64 cubics in one wave, each at most 2^12 points: the move at lane 63, the cubics at lanes 0..63 of the next wave
    st = [_CL] * 63
    cur = (0.0, 0.0)
    st.append(_mv(cur))
    for j in range(64):
        D = 7 + j % 6
        k = f32(deep_m(D, 0.6 + 0.05 * (j % 5)))
        a, b, e = _arch(cur, k, 1 if j % 2 == 0 else -1)
        a, b, e = [(f32(x), f32(y)) for x, y in (a, b, e)]
        st.append(_cu(a, b, e))
        cur = e
    st += [_ln((0.0, -100000.0)), _CL]
    out.append(Glyph("D:64-in-a-wave", st, scale=2.0 ** -12, shift=0.0, tags={"align"}))
    return out


class Lanes:
    """glyphs placed at exact lanes of the batch's waves (the family starts on a wave boundary)"""

    def __init__(self, prefix):
        self.prefix, self.glyphs, self.n = prefix, [], 0

    def add(self, name, stream, scale=UNIT, shift=0.0):
        g = Glyph(f"{self.prefix}:{name}", stream, scale, shift)
        self.glyphs.append(g)
        self.n += len(g.stream)
        return g

    def pad_to(self, lane, kind="closes"):
        """commands without items until the next command sits at `lane`"""
        k = (lane - self.n) % 64
        if not k:
            return
        if kind == "closes":
            self.add(f"pad{k}", [_CL] * k)
        elif kind == "ignored":   # curves on the empty ring of a fresh glyph
            self.add(f"ign{k}", [_qu((5, 5), (9, 9)) if i % 2 else _cu((1, 2), (3, 4), (5, 6)) for i in range(k)])
        else:                      # a mirrored glyph: no command of it takes part in the parallel rounds
            body = [_mv((10, 10)), _qu((300, 700), (600, 10)), _cu((500, -100), (200, -200), (10, 10)), _CL]
            st = (body * (k // 4 + 1))[:k]
            self.add(f"neg{k}", st, scale=-UNIT, shift=0.25)


def _quad_lev(s, lev, h_sign=1, span=400.0):
    """a quadratic from s of certain depth lev (|d| = 0.1 4^lev 0.6), chord (span, 0)"""
    dev = 0.1 * 4.0 ** lev * 0.6
    return ((s[0] + span / 2, s[1] + h_sign * dev / 2), (s[0] + span, s[1]))


def family_e():
    t = Lanes("E")
    # item totals 64 / 65 / 128 / 129 in one wave each: move + n quads of 8 items + lines, the rest of the wave without items
    for total in (64, 65, 128, 129):
        t.pad_to(0)
        nq, nl = (total - 1) // 8, (total - 1) % 8
        st, cur = [_mv((0.0, 0.0))], (0.0, 0.0)
        for j in range(nq):
            c, e = _quad_lev(cur, 6, 1 if j % 2 else -1, 300.0)
            st.append(_qu(c, e))
            cur = e
        for j in range(nl):
            cur = (cur[0] - 40.0 * (j + 1), cur[1] - 300.0)
            st.append(_ln(cur))
        st.append(_CL)
        t.add(f"total{total}", st, shift=0.125)
        t.pad_to(40, "ignored")
        t.pad_to(0, "negative")
    # far above: one quad of L = 13 (1024 items) beside parallel cubics
    t.add("L13", [_mv((-1.0e6 + 10, -9.0e5)), _qu((-1.0e6 + 9.0e5 + 5, 8.5e5), (-1.0e6 + 1.8e6, -9.0e5)),
                  _cu((8.0e5 - 20, -9.0e5 - 30), (8.0e5 - 40, -9.0e5 - 10), (8.0e5 - 60, -9.0e5 - 40)), _CL], scale=2.0 ** -12, shift=0.0)
    # an item-owning cubic at lane 0, its current point from lane 63 of the previous wave; owners at lanes 62 and 0 of
    # waves around a close at lane 63
    t.pad_to(62)
    a, b, e = _arch((100.0, 110.0), 90.0)
    t.add("cubic@lane0", [_mv((100.0, 100.0)), _ln((100.0, 110.0))] + [_cu(a, b, e), _ln((90.0, 40.0)), _CL], shift=0.25)
    t.pad_to(61)
    a, b, e = _s_curve((200.0, 100.0), 20.0, -1)
    t.add("close@63", [_mv((200.0, 100.0)), _cu(a, b, e), _CL, _mv((50.0, 50.0)), _qu(*_quad_lev((50.0, 50.0), 5)), _CL])
    # glyphs that start at lanes 0, 1 and 63, each with a curve first (an empty ring: ignored)
    for lane in (0, 1, 63):
        t.pad_to(lane)
        a, b, e = _s_curve((10.0, 10.0), 40.0)
        t.add(f"start@{lane}", [_cu(a, b, e), _qu((5, 5), (9, 9)), _mv((10.0, 10.0)), _cu(a, b, e), _ln((30.0, -60.0)), _CL,
                                _cu(a, b, e), _mv((10.0, 200.0)), _qu(*_quad_lev((10.0, 200.0), 4)), _ln((20.0, 150.0)), _CL])
    # owners separated by commands without items (closes, curves on an empty ring, a mirrored glyph); parallel and
    # sequential commands in one wave: quadratics inside the margin, bound-7 cubics
    t.pad_to(0)
    st, cur = [_mv((0.0, 0.0))], (0.0, 0.0)
    h0 = 0.05 * 4.0 ** 5
    for j in range(6):
        c, e = _quad_lev(cur, 4 + j % 3, 1, 200.0)
        st.append(_qu(c, e))
        cur = e
        margin = (cur[0] + 150.0, cur[1] + h0), (cur[0] + 300.0, cur[1])    # |d|^2 / 16^5 = tolerance^2: inside the margin
        st.append(_qu(*margin))
        cur = margin[1]
        a, b, e = _arch(cur, deep_m(7))
        st.append(_cu(a, b, e))
        cur = e
        a, b, e = _s_curve(cur, 20.0 + 10 * j, -1)
        st.append(_cu(a, b, e))
        cur = e
    st += [_ln((cur[0], cur[1] - 500.0)), _CL, _CL, _cu((1, 1), (2, 2), (3, 3)), _qu((1, 1), (2, 2))]
    t.add("mixed", st, shift=-0.125)
    t.pad_to(63, "negative")
    t.add("after-negative", [_mv((0.0, 0.0)), _qu(*_quad_lev((0.0, 0.0), 6)), _ln((100.0, -300.0)), _CL])
    return t.glyphs


def family_f():
    out = []
    # move + 200 cubics + close: the ring state of glyph commands 64..201 comes from the carry
    st, cur = [_mv((0.0, 0.0))], (0.0, 0.0)
    for j in range(200):
        shape = _s_curve if j % 3 == 0 else _arch
        a, b, e = shape(cur, 8.0 + (j % 7), 1 if (j // 25) % 2 == 0 else -1)
        st.append(_cu(a, b, e))
        cur = e
    st.append(_CL)
    out.append(Glyph("F:200-cubics", st, shift=0.0625))
    # close at glyph command 63, then a curve at 64 (ignored); a line at 63, then a curve at 64 (flattened)
    for at63 in ("close", "line"):
        st = [_mv((0.0, 0.0))]
        for j in range(1, 63):
            st.append(_ln((float(j * 7 % 50), float(j * 13 % 90))))
        st.append(_CL if at63 == "close" else _ln((60.0, -20.0)))
        a, b, e = _arch((60.0, -20.0), 30.0)
        st += [_cu(a, b, e), _ln((10.0, -50.0)), _mv((0.0, 300.0)), _ln((50.0, 300.0)), _ln((25.0, 340.0)), _CL]
        out.append(Glyph(f"F:{at63}@63", st, shift=-0.0625))
    # 1024 and 1025 commands (the ring pass keeps its state in LDS up to 1024), rings of 100 commands across the steps
    for n in (1024, 1025):
        st = []
        while len(st) < n:
            r = len(st) // 100
            o = (float(100 * (r % 4)), float(120 * (r // 4)))
            st.append(_mv(o))
            cur = o
            for j in range(98):
                if len(st) >= n - 1:
                    break
                if j % 3 == 0:
                    a, b, e = (_arch if j % 2 else _s_curve)(cur, 3.0 + j % 5, 1 if j < 49 else -1)
                    st.append(_cu(a, b, e))
                    cur = e
                elif j % 3 == 1:
                    c, e = _quad_lev(cur, 2, 1, 2.0 if j < 49 else -2.0)
                    st.append(_qu(c, e))
                    cur = e
                else:
                    cur = (cur[0], cur[1] + (1.0 if j < 49 else -1.0))
                    st.append(_ln(cur))
            st.append(_CL if len(st) < n - 1 or n == 1024 else _ln((o[0] + 5, o[1] + 50)))
        out.append(Glyph(f"F:{n}-commands", st[:n], shift=0.25))
    return out


def family_g():
    out = []
    for sc in (-UNIT, -1.0 / 32.0):
        for g in family_a() + family_b() + family_e():
            scale = sc if g.scale == UNIT else -abs(g.scale)
            out.append(Glyph(f"G{sc:g}:{g.name}", g.stream, scale=scale, shift=g.shift))
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f, "G": family_g}


def assemble(families=FAMILIES):
    """every family from a wave boundary of one batch -> (glyphs, family of each glyph); glyphs of only closes pad between
    families and in front of glyphs tagged "align"."""
    glyphs, fam, n = [], [], 0
    for name, make in families.items():
        for g in make():
            if n % 64 and (not fam or fam[-1] != name or "align" in g.tags):
                pad = Glyph(f"{name}:pad", [_CL] * (64 - n % 64))
                glyphs.append(pad)
                fam.append(name)
                n += len(pad.stream)
            glyphs.append(g)
            fam.append(name)
            n += len(g.stream)
    return glyphs, fam


def batch_arrays(glyphs):
    """-> cmd_off (uint32), device-order records [(x1, y1, x2, y2, x, y, kind)], scale, shift"""
    cmds, cmd_off = [], [0]
    for g in glyphs:
        cmds += [(c[1], c[2], c[3], c[4], c[5], c[6], c[0]) for c in g.stream]
        cmd_off.append(len(cmds))
    return (np.array(cmd_off, np.uint32), cmds, np.array([g.scale for g in glyphs]), np.array([g.shift for g in glyphs]))


# ---------------------------------------------------------------------------------------------------------------------
# classes reached (the witness)
# ---------------------------------------------------------------------------------------------------------------------

def census(glyphs, fam):
    """Counter per family of the classes its commands and waves reach"""
    per = {}
    lane_rows = []   # (family, cls, items, glyph start?, glyph index)
    for gi, (g, f) in enumerate(zip(glyphs, fam)):
        cnt = per.setdefault(f, Counter())
        mono = g.scale > 0
        cls = command_classes(g.stream, mono)
        for j, (c, items, pts, info) in enumerate(cls):
            lane_rows.append((f, c, items, j == 0, gi))
            if c.startswith("quad"):
                cnt[c + (f"-L{info}" if c == "quad-par" and info >= 9 else "")] += 1
            elif c == "cubic-par":
                D, leaves = info
                depths = [d for d, _, _, _ in leaves]
                cnt[f"cubic-par-D{D}"] += 1
                for d in set(depths):
                    cnt[f"leaf-depth{d}"] += 1
                if min(depths) < D - min(D, ITEM_DEPTH):
                    cnt[f"flat-ancestor-D{D}"] += 1
                cnt["deepest=bound" if max(depths) == D else ("slack>=2" if max(depths) <= D - 2 else "slack1")] += 1
            elif c == "cubic-seq":
                cnt[f"cubic-seq-D{min(info[0], 99)}"] += 1
            elif c == "ignored":
                cnt["ignored"] += 1
        if not mono:
            cnt["non-monotone"] += 1
        else:
            xs = [c[5] for c in g.stream] + [c[k] for c in g.stream for k in (1, 3) if c[0] in (Q, C3)]
            ys = [c[6] for c in g.stream] + [c[k] for c in g.stream for k in (2, 4) if c[0] in (Q, C3)]
            m = max((abs(v) for v in xs + ys), default=0.0)
            if m == BIG:
                cnt["m=1e6"] += 1
            elif m == NEXT:
                cnt["m=1e6+ulp"] += 1
        if len(g.stream) in (1024, 1025):
            cnt[f"commands{len(g.stream)}"] += 1
        if len(cls) > 64 and g.stream[64][0] in (Q, C3):
            cnt[f"curve@64-{cls[64][0]}-after-{cls[63][0]}"] += 1
        for j in range(64, len(cls), 64):   # a step of the context pass whose ring state comes from the carry alone
            if cls[j - 1][0] not in ("close", "ignored") and all(c[0] not in ("move", "line", "close") for c in cls[j:j + 64]):
                cnt["step-from-carry"] += 1
    for w in range(0, len(lane_rows), 64):
        rows = lane_rows[w:w + 64]
        f = rows[0][0]
        cnt = per.setdefault(f, Counter())
        tot = sum(r[2] for r in rows)
        if tot in (64, 65, 128, 129):
            cnt[f"wave-items{tot}"] += 1
        elif tot > 1024:
            cnt["wave-items>1024"] += 1
        par = any(r[2] and r[1] not in ("move", "line") for r in rows)
        seq = any(r[1] in ("quad-seq", "cubic-seq") for r in rows)
        if par and seq:
            cnt["wave-par+seq"] += 1
        if sum(r[1] in ("quad-seq", "quad-capped", "cubic-seq") for r in rows) == 1 and any(r[1] == "cubic-seq" for r in rows):
            cnt["wave-one-walker"] += 1
        if sum(r[1] == "cubic-seq" for r in rows) == 64:
            cnt["wave-64-walkers"] += 1
        for lane in (0, 1, 63):
            if len(rows) > lane and rows[lane][3] and rows[lane][4] > 0 and glyphs[rows[lane][4]].stream[0][0] in (Q, C3):
                cnt[f"glyph@lane{lane}"] += 1
        if rows[0][1] == "cubic-par" and w and lane_rows[w - 1][4] == rows[0][4] and lane_rows[w - 1][1] in ("move", "line"):
            cnt["owner@0-after-63"] += 1
        if len(rows) == 64 and rows[63][2] == 0 and rows[62][2] and w + 64 < len(lane_rows) and lane_rows[w + 64][2]:
            cnt["zero@63-between-owners"] += 1
        for j in range(1, len(rows) - 1):
            if rows[j][2] == 0 and rows[j - 1][2] and any(r[2] for r in rows[j + 1:]):
                cnt["zero-between-owners"] += 1
                break
    return per


@pytest.fixture(scope="module")
def assembled():
    return assemble()


# (family, class) -> how many cases reach it (census above): every class the families were written for, the flat
# ancestor above the item roots (flat-ancestor-D4/5/6) and every leaf depth 0..6 included
WITNESS = {
    ("A", "cubic-par-D0"): 16, ("A", "cubic-par-D1"): 32, ("A", "cubic-par-D2"): 32, ("A", "cubic-par-D3"): 32,
    ("A", "cubic-par-D4"): 32, ("A", "cubic-par-D5"): 32, ("A", "cubic-par-D6"): 32, ("A", "cubic-seq-D7"): 16,
    ("A", "deepest=bound"): 112, ("A", "leaf-depth0"): 32, ("A", "leaf-depth1"): 54, ("A", "leaf-depth2"): 64,
    ("A", "leaf-depth3"): 64, ("A", "leaf-depth4"): 64, ("A", "leaf-depth5"): 48, ("A", "leaf-depth6"): 16,
    ("A", "slack1"): 96, ("A", "wave-items128"): 2, ("A", "wave-par+seq"): 2, ("A", "zero-between-owners"): 14,
    ("A", "zero@63-between-owners"): 14,
    ("B", "cubic-par-D0"): 24, ("B", "cubic-par-D1"): 3, ("B", "cubic-par-D2"): 75, ("B", "cubic-par-D3"): 124,
    ("B", "cubic-par-D4"): 109, ("B", "cubic-par-D5"): 104, ("B", "cubic-par-D6"): 104, ("B", "deepest=bound"): 314,
    ("B", "flat-ancestor-D4"): 24, ("B", "flat-ancestor-D5"): 24, ("B", "flat-ancestor-D6"): 24,
    ("B", "leaf-depth0"): 145, ("B", "leaf-depth1"): 24, ("B", "leaf-depth2"): 113, ("B", "leaf-depth3"): 199,
    ("B", "leaf-depth4"): 201, ("B", "leaf-depth5"): 143, ("B", "leaf-depth6"): 64, ("B", "slack1"): 109,
    ("B", "slack>=2"): 120, ("B", "wave-items64"): 1, ("B", "wave-items65"): 2, ("B", "zero-between-owners"): 34,
    ("B", "zero@63-between-owners"): 33,
    ("C", "cubic-par-D4"): 2, ("C", "cubic-par-D5"): 14, ("C", "cubic-seq-D4"): 2, ("C", "cubic-seq-D5"): 14,
    ("C", "deepest=bound"): 16, ("C", "leaf-depth3"): 10, ("C", "leaf-depth4"): 16, ("C", "leaf-depth5"): 14,
    ("C", "m=1e6"): 33, ("C", "m=1e6+ulp"): 28, ("C", "owner@0-after-63"): 1, ("C", "quad-capped"): 2,
    ("C", "quad-par"): 12, ("C", "quad-par-L10"): 1, ("C", "quad-par-L11"): 1, ("C", "quad-par-L12"): 1,
    ("C", "quad-par-L13"): 1, ("C", "quad-par-L9"): 1, ("C", "quad-seq"): 14, ("C", "wave-items64"): 1,
    ("C", "wave-items>1024"): 1, ("C", "wave-par+seq"): 5, ("C", "zero-between-owners"): 5,
    ("C", "zero@63-between-owners"): 2,
    ("D", "cubic-seq-D10"): 12, ("D", "cubic-seq-D11"): 11, ("D", "cubic-seq-D12"): 11, ("D", "cubic-seq-D13"): 1,
    ("D", "cubic-seq-D14"): 1, ("D", "cubic-seq-D15"): 1, ("D", "cubic-seq-D16"): 1, ("D", "cubic-seq-D7"): 12,
    ("D", "cubic-seq-D8"): 12, ("D", "cubic-seq-D9"): 12, ("D", "curve@64-cubic-seq-after-move"): 1,
    ("D", "step-from-carry"): 1, ("D", "wave-64-walkers"): 1, ("D", "wave-one-walker"): 10,
    ("D", "zero-between-owners"): 10,
    ("E", "cubic-par-D6"): 9, ("E", "cubic-seq-D7"): 41, ("E", "deepest=bound"): 1, ("E", "flat-ancestor-D6"): 8,
    ("E", "glyph@lane0"): 1, ("E", "glyph@lane1"): 1, ("E", "glyph@lane63"): 1, ("E", "ignored"): 103,
    ("E", "leaf-depth0"): 8, ("E", "leaf-depth6"): 1, ("E", "non-monotone"): 5, ("E", "owner@0-after-63"): 1,
    ("E", "quad-par"): 57, ("E", "quad-par-L13"): 1, ("E", "quad-seq"): 38, ("E", "slack>=2"): 8,
    ("E", "wave-items128"): 1, ("E", "wave-items129"): 1, ("E", "wave-items64"): 1, ("E", "wave-items65"): 1,
    ("E", "wave-items>1024"): 1, ("E", "wave-par+seq"): 5, ("E", "zero-between-owners"): 6,
    ("E", "zero@63-between-owners"): 1,
    ("F", "commands1024"): 1, ("F", "commands1025"): 1, ("F", "cubic-par-D4"): 449, ("F", "cubic-par-D5"): 409,
    ("F", "cubic-par-D6"): 19, ("F", "curve@64-cubic-par-after-cubic-par"): 1,
    ("F", "curve@64-cubic-par-after-line"): 3, ("F", "curve@64-ignored-after-close"): 1, ("F", "deepest=bound"): 462,
    ("F", "flat-ancestor-D4"): 82, ("F", "flat-ancestor-D5"): 314, ("F", "flat-ancestor-D6"): 19, ("F", "ignored"): 1,
    ("F", "leaf-depth0"): 415, ("F", "leaf-depth3"): 62, ("F", "leaf-depth4"): 424, ("F", "leaf-depth5"): 95,
    ("F", "owner@0-after-63"): 10, ("F", "quad-par"): 675, ("F", "slack>=2"): 415, ("F", "step-from-carry"): 2,
    ("F", "zero-between-owners"): 24,
    ("G", "cubic-seq-D0"): 80, ("G", "cubic-seq-D1"): 70, ("G", "cubic-seq-D2"): 214, ("G", "cubic-seq-D3"): 312,
    ("G", "cubic-seq-D4"): 282, ("G", "cubic-seq-D5"): 272, ("G", "cubic-seq-D6"): 290, ("G", "cubic-seq-D7"): 114,
    ("G", "ignored"): 206, ("G", "non-monotone"): 1588, ("G", "quad-seq"): 192, ("G", "wave-one-walker"): 4,
}


def test_restated_rings_equal_the_oracle(oracle, assembled):
    """the restated point counts put through RingBuilder's rules give the oracle's rings, glyph for glyph; every parallel
    cubic keeps its depth bound and its leaves have distinct first candidates, in order"""
    glyphs, _ = assembled
    for g in glyphs:
        cls = command_classes(g.stream)
        want = [len(r) for r in oracle.build_rings(g.stream, cap=1 << 18, max_rings=1 << 12)]
        assert ring_lengths(g.stream, cls) == want, g.name
        for c, _, _, info in cls:
            if c == "cubic-par":
                D, leaves = info
                assert max(d for d, _, _, _ in leaves) <= D, g.name
                cand = first_candidates(leaves, D)
                assert cand == sorted(set(cand)) and cand[-1] < 1 << D, g.name


def test_witness_every_class_is_reached(assembled):
    per = census(*assembled)
    got = {(f, k): v for f, cnt in per.items() for k, v in cnt.items()}
    assert got == WITNESS, {k: (got.get(k), WITNESS.get(k)) for k in set(got) | set(WITNESS) if got.get(k) != WITNESS.get(k)}
    for D in (4, 5, 6):   # a leaf above the item roots: one point from 2^(D-3) items (outline_kernels.hip, wave_parallel_points)
        assert got[("B", f"flat-ancestor-D{D}")] >= 20 and got[("F", f"flat-ancestor-D{D}")] >= 10
    for d in range(7):
        assert got[("A", f"leaf-depth{d}")] and got[("B", f"leaf-depth{d}")]
    assert all(got[("D", f"cubic-seq-D{D}")] for D in range(7, 17))
    assert all(got[("C", f"quad-par-L{lev}")] == 1 for lev in range(9, 14))
    assert all(got[("E", f"wave-items{t}")] == 1 for t in (64, 65, 128, 129, ">1024"))


# ---------------------------------------------------------------------------------------------------------------------
# a CFF font of these shapes
# ---------------------------------------------------------------------------------------------------------------------

CFF_FIRST_CP = 0x100


def _q256(v):
    return round(v * 256.0) / 256.0


def cff_programs():
    """Type 2 charstrings of families A, B, F and D (bounds 7..10: the operands of deeper ones leave +-32767): every
    coordinate on 1/256 (exact in 16.16 operands and in f32), relative operands; a ring ends at the next rmoveto or at
    endchar (the readers emit close() there), commands on an empty ring have no charstring form and are left out"""
    keep = family_a() + family_b() + [g for g in family_d() if g.name in ("D:bound7", "D:bound8", "D:bound9", "D:bound10")] + \
        family_f()
    progs = []
    for g in keep:
        prog, cur, open_ = [], (0.0, 0.0), False
        for k, x1, y1, x2, y2, x, y in g.stream:
            if k == Q:                 # raised to a cubic
                x1, y1, x2, y2 = cur[0] + 2 * (x1 - cur[0]) / 3, cur[1] + 2 * (y1 - cur[1]) / 3, x + 2 * (x1 - x) / 3, y + 2 * (y1 - y) / 3
                k = C3
            pts = {M: [(x, y)], L: [(x, y)], C3: [(x1, y1), (x2, y2), (x, y)], Z: []}[k]
            if k == Z:
                open_ = False
                continue
            if k in (Q, C3) and not open_:
                continue
            if k == L and not open_:   # a line that starts a ring: a move in CFF
                k = M
            ops = []
            for px, py in pts:
                px, py = _q256(px), _q256(py)
                ops += [px - cur[0], py - cur[1]]
                cur = (px, py)
            prog += ops + [{M: "rmoveto", L: "rlineto", C3: "rrcurveto"}[k]]
            open_ = True
        progs.append((g.name, prog + ["endchar"]))
    return progs


def build_cff_font():
    from fontTools.misc.psCharStrings import T2CharString
    from test_cff_outlines import _build
    progs = cff_programs()
    names = [".notdef"] + [f"g{i}" for i in range(len(progs))]
    cs = {".notdef": T2CharString(program=[0, "hmoveto", "endchar"])}
    for n, (_, p) in zip(names[1:], progs):
        cs[n] = T2CharString(program=[v if isinstance(v, str) or v != int(v) else int(v) for v in p])
    cmap = {CFF_FIRST_CP + i: n for i, n in enumerate(names[1:])}
    return _build(names, cmap, cs, {n: 600 + 7 * (i % 50) for i, n in enumerate(names)})


@pytest.fixture(scope="module")
def shapes_cff():
    pytest.importorskip("fontTools")
    return build_cff_font()


def test_cff_font_carries_the_shapes(oracle, shapes_cff):
    """the oracle's reader gives back the intended commands (on 1/256), and the deep cubics reach their bounds"""
    f = oracle.Font(shapes_cff)
    progs = cff_programs()
    assert len(f.codepoints()) == len(progs)
    bounds = Counter()
    for i, (name, _) in enumerate(progs):
        seq = f.outline(f.glyph_index(CFF_FIRST_CP + i))
        cls = command_classes([(k, x1, y1, x2, y2, x, y) for k, x1, y1, x2, y2, x, y in seq])
        for c, _, _, info in cls:
            if c.startswith("cubic"):
                bounds[(c, info[0])] += 1
    assert all(bounds[("cubic-seq", D)] >= 1 for D in (7, 8, 9, 10)), bounds
    assert all(bounds[("cubic-par", D)] >= 20 for D in range(7)), bounds


def test_cff_shapes_host_segments_equal_oracle(oracle, vg, shapes_cff):
    """FontManager.build_batch (the host's flatten_cubic, csrc/host/geometry.hpp) gives the oracle's segments and rects"""
    m = vg.FontManager(True)
    fid = m.add_font_data("Flatten Shapes", shapes_cff)
    hb = m.build_batch(fid)
    b = hb.batch
    font = oracle.Font(shapes_cff)
    g = 0
    for cp in sorted(int(c) for c in font.codepoints()):
        r = font.prepare_glyph(cp)
        if r is None or not r[0].has_bitmap:
            continue
        info, segs = r
        assert int(hb.ids[g]) == cp
        a, e = int(b.seg_off[g]), int(b.seg_off[g + 1])
        got = np.stack([b.seg_sx[a:e], b.seg_sy[a:e], b.seg_ex[a:e], b.seg_ey[a:e]], axis=1)
        assert got.tobytes() == segs.tobytes(), hex(cp)
        assert (int(b.x0[g]), int(b.y0[g]), int(b.w[g]), int(b.h[g])) == (info.x0, info.y0, info.w, info.h), hex(cp)
        g += 1
    assert g == b.n_glyphs and g > 400


def test_cff_shapes_dummy_pbf_equal_oracle(oracle, vg, shapes_cff):
    mgr = vg.FontManager(True)
    fid = mgr.add_font_data("Flatten Shapes", shapes_cff)
    w = vg.DummyWriter()
    mgr.render_glyphs(w, vg.Renderer.new_dummy())
    font = oracle.Font(shapes_cff)
    n = 0
    for blk in range(256):
        want, k, _ = oracle.render_block([font], fid, blk * 256, oracle.DUMMY)
        assert w.files[f"{fid}/{blk * 256}-{blk * 256 + 255}.pbf"] == want, blk
        n += k
    assert n == len(cff_programs())
