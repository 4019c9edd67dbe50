"""GPU: the raster kernel (sdf_tiles_span, csrc/sdf_span_kernel.inc) and the two planners that feed it (build_descs_and_tiles
in work_list.cpp on the host, outline_plan in outline_plan_kernels.hip on the device, both on the policy of csrc/work_plan.h) at the
regimes set by a glyph's width and segment count, against the oracle (BRUTE and PRECISE) under both product variants (0: spans,
1: brute force).

The routing is restated below (fits, the choice of the span length T from span_max and span_budget, the brute-force class, the
span count per glyph).  Every host-plan case carries a witness: vgsdf_batch_stats' n_tiles under variant 0 equals the restated
span count (under variant 1 the 256-pixel tile count), so each case is shown to land in the regime it was written for.

  width sweep          every T of the width table, its non-monotone edges +-3, the widths whose histogram is the fullest
  device plan          the same widths as command streams through outlines_prepare / outlines_render
  chunk count x budget n_seg = 256 c and 256 c + 1 in batches of 2047 (budget 8) and 2048 (budget 16) glyphs
  forced span lengths  VGSDF_SPAN_MAX = 1, 2, 3 and VGSDF_SPAN_BUDGET = 1 give the default bytes (child processes)
  crossing pool        the first wave's (segment, row) crossings at QCAP = 256 / 257 and far above
  filter guards        far vertices at Mc = 4096 (bounded) and 1e6 (sane) +- 0.05 % / 0.5 %, in chunks 0, 1, 2
  int32 edges          x0, y0 at -2^31 and 2^31 - w - 1, edges on 1/64 px, far parts at 2^23 / 2^24
  2^24 segments        the segment-count route to brute force, both sides"""
import hashlib
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_front_end_regimes import _stream

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# ---------------------------------------------------------------------------------------------------------------------
# the routing, restated
# ---------------------------------------------------------------------------------------------------------------------

DELTA_CAP = 2048   # winding histogram cells of the span kernel (vgsdf_filtered_delta_cap)
TILE = 256         # pixels per tile
CHUNK = 256        # segments per LDS chunk (FCHUNK)
SPAN_TILES = 4     # the largest span the kernel sweeps
QCAP = 256         # pooled (segment, row) crossings per wave


def fits(w, T):
    """rows touched by T consecutive tiles, times a row stride of at most w + 2, fit the histogram"""
    return ((TILE * T - 2) // w + 2) * (w + 2) <= DELTA_CAP


def span_budget(n_glyphs):
    return 8 if n_glyphs < 2048 else 16


def span_length(w, n_seg, n_glyphs=1, span_max=SPAN_TILES, budget=None):
    """T of the span list; 0: the brute-force class (histogram does not fit one tile, or >= 2^24 segments)"""
    if not fits(w, 1) or n_seg >= 1 << 24:
        return 0
    budget = span_budget(n_glyphs) if budget is None else budget
    chunks = -(-n_seg // CHUNK)
    T = min(span_max, max(1, budget // max(chunks, 1)))
    while T > 1 and not fits(w, T):
        T -= 1
    return T


def span_count(w, h, T):
    """work-list entries of a glyph: spans of T tiles (brute force, T = 0: one per 256-pixel tile)"""
    t256 = -(-(w * h) // TILE)
    return t256 if T == 0 else -(-t256 // T)


def stride(w):
    return (w + 1) | 1   # the kernel's histogram row: w + 1 cells padded to an odd count


def hist_cells(w, h, T):
    """the largest rows x stride over the glyph's actual spans (p0 = k 256 T), as the kernel sizes s_delta"""
    npix, n = w * h, TILE * T
    p0 = np.arange(0, npix, n, dtype=np.int64)
    pe = np.minimum(p0 + n, npix)
    return int(((pe - 1) // w - p0 // w + 1).max()) * stride(w)


def hist_reachable(w, T):
    """the largest rows x stride any span of T tiles can reach at width w (its start column cycles with k 256 T mod w)"""
    n = TILE * T
    a = (np.arange(w // math.gcd(n, w), dtype=np.int64) * n) % w
    return int(((a + n - 1) // w + 1).max()) * stride(w)


def pick_height(w, T, lo=4):
    """the smallest height >= lo with >= 3 full spans, a partial last span (unless w is a multiple of the span: 768 at T = 3)
    and a span whose histogram is the fullest the width can reach (searched, not guessed)"""
    if T == 0:
        return max(lo, 7)
    n = TILE * T
    want = hist_reachable(w, T)
    for h in range(max(lo, -(-3 * n // w) + 1), 1 << 16):
        if ((w * h) % n or w % n == 0) and hist_cells(w, h, T) == want:
            return h
    raise AssertionError((w, T))


def plan_tiles(ctx, batch, variant=0):
    """n_tiles of vgsdf_batch_stats: the work-list entries the plan made for `batch` under `variant`"""
    ctx.set_variant(variant)
    db = ctx.upload(batch)
    try:
        return db.stats()["n_tiles"]
    finally:
        db.free()
        ctx.set_variant(0)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures and checks
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def oracle_bytes(oracle, batch, modes):
    want = None
    for mode in modes:
        got, _ = oracle.sdf_render_batch(batch, mode, 0)
        if want is None:
            want = got
        else:
            assert np.array_equal(got, want), "the oracle's modes disagree"
    return want


def run_both(oracle, vg, ctx, batch, modes):
    """both product variants equal the oracle in every mode of `modes` -> the bytes"""
    want = oracle_bytes(oracle, batch, modes)
    for variant in (0, 1):
        ctx.set_variant(variant)
        got = ctx.render_batch(batch)
        diff = np.flatnonzero(got != want)
        if diff.size:
            g = int(np.searchsorted(batch.out_off, diff[0], side="right")) - 1
            p = int(diff[0] - batch.out_off[g])
            pytest.fail(f"variant {variant}: {diff.size} bytes differ; first: glyph {g} (x0 {batch.x0[g]}, y0 {batch.y0[g]}, "
                        f"w {batch.w[g]}, h {batch.h[g]}, {batch.seg_off[g + 1] - batch.seg_off[g]} segments), pixel {p} "
                        f"(span of 1024 px {p // 1024}, tile {p // 256}), got {got[diff[0]]} want {want[diff[0]]}")
    ctx.set_variant(0)
    return want


def test_the_restated_constants_are_the_kernels(vg):
    assert vg.load_library().vgsdf_filtered_delta_cap() == DELTA_CAP


def test_the_restated_width_table():
    """the width -> T table of one chunk (the mapping is not monotone: 511 -> 3, 681 -> 2), and where the histogram is fullest"""
    edges = {}
    prev = None
    for w in range(1, 1100):
        T = span_length(w, 9)
        if T != prev:
            edges[w] = T
            prev = T
    assert edges == {1: 2, 2: 3, 3: 4, 511: 3, 512: 4, 681: 2, 767: 3, 1023: 0}
    # exact-fit widths: the planner's measure rows x (w + 2) within 4 cells of DELTA_CAP
    bound = {w: ((TILE * span_length(w, 9) - 2) // w + 2) * (w + 2) for w in range(1, 1023)}
    assert tuple(sorted(w for w, b in bound.items() if b >= DELTA_CAP - 4)) == EXACT_FIT
    # the kernel's odd stride (w + 1) | 1 is one cell below w + 2 for even w: the fullest it gets is 2046 at w = 1021-1022
    assert max(hist_reachable(w, span_length(w, 9)) for w in range(1, 1023)) == 2046


# ---------------------------------------------------------------------------------------------------------------------
# width sweep (host plan)
# ---------------------------------------------------------------------------------------------------------------------

EDGES = list(range(508, 515)) + list(range(677, 685)) + list(range(763, 771)) + list(range(1019, 1027))
FULLEST = [507, 508, 509, 510, 675, 676, 677, 678, 679, 680] + list(range(1013, 1023))
STRIDE = [7, 17, 40, 101, 256, 333, 450, 530, 600, 650, 700, 730, 800, 901, 990, 1100, 1500]
WIDTHS = sorted(set(range(1, 7)) | set(EDGES) | set(FULLEST) | set(STRIDE))
EXACT_FIT = (509, 510, 680, 1020, 1021, 1022)   # the planner's measure rows x (w + 2) within 4 cells of DELTA_CAP


def hist_outline(w, h):
    """rings (px, relative to the rect's corner) that stress the winding histogram of a w x h rect: vertices on pixel centres
    (x.5) and on sample rows, a long near-vertical edge crossing left of column 0 in the low rows, one crossing right of
    column w - 1, a notch to the middle, and a hole"""
    mx, my = (w >> 1) + 0.5, (h >> 1) + 0.5
    outer = [(-1.25, 0.5), (w + 0.75, 0.5), (mx, my), (w - 0.5, h - 0.5), (0.5, h - 0.5)]
    xa, xb = (w // 10) + 0.5, (3 * w // 10) + 0.75
    ya, yb = (h // 10) + 0.5, (4 * h // 10) + 1.5
    hole = [(xa, ya), (xa, yb), (xb + 0.25, yb), (xb, ya)]   # (quarter pixels: exact in the front-end's f32 commands)
    return [np.array(outer), np.array(hole)]


def sweep_glyphs():
    """one glyph per width of WIDTHS, at a height picked by pick_height: (segs, x0, y0, w, h)"""
    out = []
    for w in WIDTHS:
        h = pick_height(w, span_length(w, 9))
        x0, y0 = -(w % 7), (w % 5) - 2
        segs = np.concatenate([ring(r) for r in hist_outline(w, h)])
        segs[:, [0, 2]] += x0
        segs[:, [1, 3]] += y0
        out.append((segs, x0, y0, w, h))
    return out


@pytest.fixture(scope="module")
def sweep(vg):
    glyphs = sweep_glyphs()
    return glyphs, vg.make_batch(glyphs)


def test_width_sweep_picks_the_intended_heights(sweep):
    """each glyph reaches the fullest histogram its width allows, over >= 3 spans with a partial last one"""
    glyphs, _ = sweep
    for segs, _, _, w, h in glyphs:
        T = span_length(w, len(segs))
        if T == 0:
            assert w >= 1023
            continue
        assert hist_cells(w, h, T) == hist_reachable(w, T) <= DELTA_CAP and w * h > 3 * TILE * T
        assert (w * h) % (TILE * T) or w % (TILE * T) == 0
        if w in EXACT_FIT:   # the worst span the planner admits is rendered: 2042-2046 of the 2048 cells (odd stride)
            assert hist_cells(w, h, T) == ((TILE * T - 2) // w + 2) * stride(w) >= DELTA_CAP - 6, w


def test_width_sweep(oracle, vg, ctx, sweep):
    """every regime of the width table: the bytes of both variants are the oracle's, and the host plan made the restated span
    count for each glyph alone (a wrong T cannot hide in a sum)"""
    glyphs, batch = sweep
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    bad = {}
    for g in glyphs:
        segs, _, _, w, h = g
        one = vg.make_batch([g])
        want = (span_count(w, h, span_length(w, len(segs))), span_count(w, h, 0))
        got = (plan_tiles(ctx, one, 0), plan_tiles(ctx, one, 1))
        if got != want:
            bad[w] = (got, want)
    assert not bad, bad                                  # {w: ((n_tiles variant 0, variant 1), restated)}


SPAN_CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, "tests")
from conftest import load_product
import test_gpu_span_regimes as S
vg = load_product()
glyphs = S.sweep_glyphs()
c = vg.SdfContext(0)
out = c.render_batch(vg.make_batch(glyphs))
tiles = [S.plan_tiles(c, vg.make_batch([g]), 0) for g in glyphs]
c.close()
print(json.dumps({"sha": hashlib.sha256(out.tobytes()).hexdigest(), "tiles": tiles}))
'''


@pytest.mark.parametrize("env", ({"VGSDF_SPAN_MAX": "1"}, {"VGSDF_SPAN_MAX": "2"}, {"VGSDF_SPAN_MAX": "3"},
                                 {"VGSDF_SPAN_BUDGET": "1"}), ids=lambda e: "=".join(next(iter(e.items()))))
def test_forced_span_lengths_give_the_default_bytes(oracle, vg, ctx, sweep, env):
    """the switches are read once per process: each setting renders the width sweep in a child, whose span counts follow the
    restatement under the forced span_max / budget and whose bytes are the default run's"""
    glyphs, batch = sweep
    want = hashlib.sha256(oracle_bytes(oracle, batch, (oracle.BRUTE,)).tobytes()).hexdigest()
    cp = subprocess.run([sys.executable, "-c", SPAN_CHILD], cwd=ROOT, env=dict(os.environ, **env), capture_output=True,
                        text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr[-2000:]
    got = json.loads(cp.stdout.strip().splitlines()[-1])
    span_max, budget = int(env.get("VGSDF_SPAN_MAX", SPAN_TILES)), int(env["VGSDF_SPAN_BUDGET"]) if "VGSDF_SPAN_BUDGET" in env else None
    restated = [span_count(w, h, span_length(w, len(s), 1, span_max, budget)) for s, _, _, w, h in glyphs]
    assert got["tiles"] == restated
    assert got["sha"] == want


# ---------------------------------------------------------------------------------------------------------------------
# the same widths through the device plan
# ---------------------------------------------------------------------------------------------------------------------

def test_width_sweep_through_the_device_plan(oracle, vg):
    """command streams of straight lines whose front-end rects have the sweep's widths (and picked heights): outline_plan's
    classify routes them; its span count is not visible at the C ABI, so the bytes are the witness -- the oracle's, and
    vgsdf_render_batch's (host plan) over the segments the front-end produced"""
    targets = [w for w in WIDTHS if w >= 10]
    streams, rings_of = [], []
    for w in targets:
        h = pick_height(w, span_length(w, 9), lo=12)
        rings = hist_outline(w - 9, h - 6)          # bbox [-1.25, w - 8.25] x [0.5, h - 6.5]: floor / ceil + 3 px each side
        streams.append(_stream(rings, 1.0))
        rings_of.append((rings, w, h))
    cmds = [(c[1], c[2], c[3], c[4], c[5], c[6], c[0]) for st in streams for c in st]
    cmd_off = np.concatenate([[0], np.cumsum([len(st) for st in streams])]).astype(np.uint32)
    n = len(streams)
    c = vg.SdfContext(0)
    try:
        rects, ob, ns = c.outlines_prepare(cmd_off, np.array(cmds, dtype=vg.OUTLINE_CMD_DTYPE), np.ones(n), np.zeros(n))
        out = c.outlines_render()
        seg_off, segs = c.outlines_segments()
        glyphs = []
        for g, (rings, w, h) in enumerate(rings_of):
            r = rects[g]
            assert (int(r["has_raster"]), int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])) == (1, -5, -3, w, h), g
            mine = np.concatenate([ring(p) for p in rings])
            assert segs[seg_off[g]:seg_off[g + 1]].tobytes() == mine.tobytes(), w
            glyphs.append((mine, -5, -3, w, h))
        batch = vg.make_batch(glyphs)
        assert len(out) == ob == batch.out_bytes and ns == len(batch.seg_sx)
        want = oracle_bytes(oracle, batch, (oracle.BRUTE, oracle.PRECISE))
        host = c.render_batch(batch)
        bad = {w: (int(np.count_nonzero(out[a:b] != want[a:b])), int(np.count_nonzero(host[a:b] != want[a:b])))
               for w, a, b in zip(targets, batch.out_off[:-1], batch.out_off[1:])
               if not (np.array_equal(out[a:b], want[a:b]) and np.array_equal(host[a:b], want[a:b]))}
        assert not bad, bad                          # {w: (device-plan bytes unlike the oracle's, host-plan bytes unlike it)}
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# chunk count x span budget
# ---------------------------------------------------------------------------------------------------------------------

TINY = (ring([(1.0, 1.0), (3.0, 1.25), (2.0, 3.0)]), 0, 0, 4, 4)   # 16 px: one span of the padding


def ellipse_glyph(n_seg):
    """a 24 x 127 rect (12 tiles: T = 4, 3, 2, 1 give 3, 4, 6, 12 spans) holding one ring of n_seg segments, tall enough that
    its chunks have boxes of their own (the box test takes glyphs of more than 512 segments)"""
    a = np.linspace(0, 2 * np.pi, n_seg, endpoint=False)
    pts = np.stack([12.0 + 9.5 * np.cos(a), 63.5 + 60.0 * np.sin(a)], 1)
    return (ring(pts), 0, 0, 24, 127)


@pytest.mark.parametrize("n_glyphs", (2047, 2048))
@pytest.mark.parametrize("n_seg", [256 * c + d for c in (1, 2, 4, 5, 8) for d in (0, 1)])
def test_chunk_count_against_the_span_budget(oracle, vg, ctx, n_glyphs, n_seg):
    """T = min(4, budget // chunks) on both sides of 2, 4, 5, 8 chunks, under budget 8 (2047 glyphs) and 16 (2048 glyphs):
    one glyph of interest padded with tiny glyphs of one span each"""
    big = ellipse_glyph(n_seg)
    batch = vg.make_batch([big] + [TINY] * (n_glyphs - 1))
    T = span_length(24, n_seg, n_glyphs)
    assert T == {8: {256: 4, 257: 4, 512: 4, 513: 2, 1024: 2, 1025: 1, 1280: 1, 1281: 1, 2048: 1, 2049: 1},
                 16: {256: 4, 257: 4, 512: 4, 513: 4, 1024: 4, 1025: 3, 1280: 3, 1281: 2, 2048: 2, 2049: 1}}[span_budget(n_glyphs)][n_seg]
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == span_count(24, 127, T) + (n_glyphs - 1)
    assert plan_tiles(ctx, batch, 1) == span_count(24, 127, 0) + (n_glyphs - 1)


# ---------------------------------------------------------------------------------------------------------------------
# crossing pool
# ---------------------------------------------------------------------------------------------------------------------

def first_ge(v, c, a, b):
    """smallest integer n in [a, b] with n + c >= v (b if none) -- the kernel's row bracket"""
    n = math.ceil(v - c)
    n = min(max(n, a), b)
    if n > a and (n - 1) + c >= v:
        n -= 1
    elif n < b and n + c < v:
        n += 1
    return n


def wave_crossings(segs, y0, w, h, T, span, wave):
    """(segment, row) crossings of the 64 segments of `wave` (chunk 0) with the sample rows of `span`, as the stage counts them"""
    p0 = span * TILE * T
    p_end = min(p0 + TILE * T, w * h)
    y_hi, y_lo = h - 1 - p0 // w, h - 1 - (p_end - 1) // w
    y0c = y0 + 0.5
    total = 0
    for vx, vy, wx, wy in segs[64 * wave:64 * wave + 64]:
        lo, hi = min(vy, wy), max(vy, wy)
        if vy != wy and hi > y_lo + y0c and lo <= y_hi + y0c:
            total += max(0, first_ge(hi, y0c, y_lo, y_hi + 1) - first_ge(lo, y0c, y_lo, y_hi + 1))
    return total


def pool_glyph(w, n_pairs, h=700):
    """a w x h glyph whose first 64 segments zig-zag through span 0's rows (up, or up then down when the band is short) so that
    they cross exactly n_pairs of them; the ring closes through a few segments in the next wave"""
    T = span_length(w, 80)
    band_lo = h - 1 - ((TILE * T - 1) // w)        # lowest sample row of span 0 (relative)
    up = 64 if h - band_lo > n_pairs + 2 else 32   # (short band: 32 segments up, 32 down over the same rows)
    steps = [4.0] * 64
    steps[0] += n_pairs - 256
    y = band_lo + 0.25
    pts = [(0.5, y)]
    for k, s in enumerate(steps):
        y += s if k < up else -s
        pts.append((0.5 if k % 2 else w - 0.5, y))
    pts += [(w - 0.25, h + 2.0), (w + 0.5, -2.0), (0.25, -2.0)]
    return ring(pts), T


@pytest.mark.parametrize("w", (3, 7))
def test_crossing_pool_at_its_capacity(oracle, vg, ctx, w):
    """QCAP = 256 pooled crossings per wave: the first wave crosses exactly 256 rows of span 0 (pooled), 257 (every lane walks
    its own rows), and a two-edge glyph whose first wave crosses every row of every span twice (far above the pool)"""
    glyphs, counts = [], []
    for n_pairs in (256, 257):
        segs, T = pool_glyph(w, n_pairs)
        counts.append(wave_crossings(segs, 0, w, 700, T, 0, 0))
        glyphs.append((segs, 0, 0, w, 700))
    assert counts == [QCAP, QCAP + 1]
    box = ring([(-0.6, -1.0), (w - 0.3, -1.0), (w - 0.3, 701.0), (-0.6, 701.0)])
    slant = ring([(0.5, -1.0), (w + 0.5, -1.0), (w - 1.0, 701.0), (-0.5, 701.0)])
    for segs in (box, slant):
        T = span_length(w, len(segs))
        assert wave_crossings(segs, 0, w, 700, T, 0, 0) == 2 * (1 + (TILE * T - 1) // w) > QCAP
        glyphs.append((segs, 0, 0, w, 700))
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == sum(span_count(w, 700, span_length(w, len(g[0]))) for g in glyphs)


# ---------------------------------------------------------------------------------------------------------------------
# filter guards
# ---------------------------------------------------------------------------------------------------------------------

WIN = 24   # the window: a 24 x 24 rect at (0, 0); the filter's origin is its integer middle (12, 12)


def near_ring(n, r, reverse=False, cy=12.0):
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    pts = np.stack([12.0 + r * np.cos(a) + 0.3 * np.sin(5 * a), cy + r * np.sin(a)], 1)
    return ring(pts[::-1] if reverse else pts)


def spike(mc):
    """a thin triangle from the near part of the outline to a vertex at x = 12 + D, D set so that the chunk's coordinate bound
    (f32, rounded up by 1.00001) is mc; its long edges cross the window"""
    d = mc / 1.00001
    return ring([(4.3, 9.1), (12.0 + d, 12.37), (4.1, 10.9)])


def coordinate_bound(segs, ox=12.0, oy=12.0):
    """Mc of a chunk as the stage forms it: f32 coordinates relative to the origin, end point as v + d, times 1.00001f; at least
    mpix = 0.5 max(w, h) + 1"""
    f = np.float32
    vx, vy = (segs[:, 0] - ox).astype(f), (segs[:, 1] - oy).astype(f)
    dx, dy = (segs[:, 2] - segs[:, 0]).astype(f), (segs[:, 3] - segs[:, 1]).astype(f)
    m = np.max(np.maximum(np.maximum(np.abs(vx), np.abs(vy)), np.maximum(np.abs(vx + dx), np.abs(vy + dy))))
    return max(f(m) * f(1.00001), f(0.5 * WIN + 1.0))


def guard_glyph(layout, mc):
    """chunks of 256 segments (the last one shorter) in `layout`: "near" -- rings around the window's middle; "spike" -- the far
    triangle and near rings; "away" -- a ring 50 px above the window (every span's box test skips it) -> (segs, chunks)"""
    chunks = []
    for k, kind in enumerate(layout):
        if kind == "near":
            chunks.append(near_ring(256, 9.0 - 2.5 * (k % 2), reverse=k % 2 == 1))
        elif kind == "away":
            chunks.append(near_ring(256, 4.0, cy=12.0 + 50.0 + WIN))
        elif kind == "spike":
            chunks.append(np.concatenate([spike(mc), near_ring(253, 6.0, reverse=True)]))
        else:
            chunks.append(spike(mc))
    return np.concatenate(chunks), chunks


GUARD_LAYOUTS = {
    "chunk0": ("spike", "near"),
    "chunk1": ("near", "spike_only"),
    "chunk2_behind_a_skipped_chunk": ("near", "away", "spike"),
    "chunk1_then_near": ("near", "spike", "near"),
}


@pytest.mark.parametrize("layout", list(GUARD_LAYOUTS))
def test_filter_guards(oracle, vg, ctx, layout):
    """bounded (Mc < 4096) and sane (Mc < 1e6) on both sides of each threshold, by 0.05 % and 0.5 %, with the far vertex in
    chunk 0, in chunk 1, in chunk 2 behind a chunk the box test skips, and in chunk 1 before a near chunk whose bound is reset
    to mpix; the window shows the near part"""
    glyphs, sides = [], []
    for thr in (4096.0, 1.0e6):
        for f in (-0.005, -0.0005, 0.0005, 0.005):
            segs, chunks = guard_glyph(GUARD_LAYOUTS[layout], thr * (1 + f))
            bounds = [coordinate_bound(c) for c in chunks]
            far = [k for k, kind in enumerate(GUARD_LAYOUTS[layout]) if kind.startswith("spike")]
            sides.append([bool(bounds[k] < thr) for k in far] + [bool(bounds[k] < 4096.0) for k in range(len(chunks)) if k not in far])
            assert sides[-1] == [f < 0] + [True] * (len(chunks) - 1), (thr, f, bounds)
            glyphs.append((segs, 0, 0, WIN, WIN))
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    n = len(glyphs[0][0])
    T = span_length(WIN, n, len(glyphs))
    assert plan_tiles(ctx, batch, 0) == len(glyphs) * span_count(WIN, WIN, T)
    assert (n > 2 * CHUNK) == (len(GUARD_LAYOUTS[layout]) > 2)     # the layouts of three chunks take the box test


# ---------------------------------------------------------------------------------------------------------------------
# coordinates at the edge of int32
# ---------------------------------------------------------------------------------------------------------------------

def edge_outline(k, w, h):
    """a box and a hole whose axis-aligned edges sit on multiples of 1/64 px (32 d on a byte boundary for many pixels) and two
    slanted edges, relative to the rect's corner"""
    o = k / 64.0
    box = [(2 + o, 2 + o), (w - 3 + o, 2 + o), (w - 3 + o, h - 4 + o), (2 + o, h - 4 + o)]
    hole = [(5 + o, 5.5), (5 + o, h - 7.5), (w - 6.5, h - 7.5 + o), (w - 6.5 + 3 * o, 5.5)]
    return [np.array(box), np.array(hole)]


@pytest.mark.parametrize("far", (0.0, 2.0 ** 23, 2.0 ** 24))
def test_int32_edges(oracle, vg, ctx, far):
    """x0 and y0 at -2^31 and at 2^31 - w - 1 (mabs0, x0c and the rows' sample positions at the end of int32), edges on 1/64
    px; far != 0: a ring that far from the origin in the same chunk (no usable f32 bound: every segment exact)"""
    w, h = 22, 17
    lo, hi = -(2 ** 31), 2 ** 31 - w - 1
    glyphs = []
    for x0, y0 in ((lo, lo), (hi, hi), (lo, hi), (hi, lo), (lo + 3, 0), (0, hi - 5)):
        for k in range(0, 64, 7):
            rings = edge_outline(k, w, h)
            if far:
                d = far if x0 < 0 else -far      # (toward zero: the far part stays inside the f64 grid of the near part)
                rings.append(np.array([(12.0 + d, 8.0), (12.5 + d, 9.0), (11.0 + d, 10.0)]))
            segs = np.concatenate([ring(r) for r in rings])
            segs[:, [0, 2]] += x0
            segs[:, [1, 3]] += y0
            glyphs.append((segs, x0, y0, w, h))
            if far:
                assert coordinate_bound(segs - [x0, y0, x0, y0], 11.0, 8.0) > 1.0e6
    batch = vg.make_batch(glyphs)
    assert int(batch.x0.min()) == lo and int(batch.x0.max()) + w == 2 ** 31 - 1
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == sum(span_count(w, h, span_length(w, len(g[0]), len(glyphs))) for g in glyphs)


# ---------------------------------------------------------------------------------------------------------------------
# 2^24 segments
# ---------------------------------------------------------------------------------------------------------------------

def test_the_segment_count_route_to_brute_force(oracle, vg, ctx):
    """one glyph of 2^24 - 1 segments (the span kernel, 65 536 chunks, T = 1) and one of 2^24 (brute force) on a 32 x 32 rect: a
    triangle in the rect, the rest short horizontal segments 200-300 px above it.  Those cross no sample row and lie far beyond
    the saturation distance of every pixel, so the expected bytes are the oracle's for the triangle; that they change nothing is
    checked on the triangle plus 4096 of them (the oracle needs over a minute per glyph for all 2^24).  512 MB of segments per
    glyph on the host and on the device, one glyph at a time.  Both spans and brute force make 4 entries here, so the bytes
    are the witness of the route.  About 10 s in all, most of it building the host arrays."""
    near = ring([(6.5, 5.5), (26.25, 9.5), (12.5, 27.5)])
    want = oracle_bytes(oracle, vg.make_batch([(near, 0, 0, 32, 32)]), (oracle.BRUTE, oracle.PRECISE))
    for n_seg in ((1 << 24) - 1, 1 << 24):
        assert span_length(32, n_seg) == (1 if n_seg < 1 << 24 else 0)
        i = np.arange(n_seg - len(near), dtype=np.float64)
        sx = 2.0 + (i % 4096) * (28.0 / 4096)
        sy = 200.0 + np.floor(i / 4096) * (100.0 / 4096)
        segs = np.empty((n_seg, 4))
        segs[:len(near)] = near
        segs[len(near):, 0], segs[len(near):, 1], segs[len(near):, 2], segs[len(near):, 3] = sx, sy, sx + 0.004, sy
        del i, sx, sy
        sample = np.concatenate([near, segs[len(near)::4096]])
        assert np.array_equal(oracle_bytes(oracle, vg.make_batch([(sample, 0, 0, 32, 32)]), (oracle.BRUTE, oracle.PRECISE)), want)
        batch = vg.make_batch([(segs, 0, 0, 32, 32)])
        del segs
        assert len(batch.seg_sx) == n_seg
        for variant in (0, 1):
            ctx.set_variant(variant)
            got = ctx.render_batch(batch)
            assert np.array_equal(got, want), (n_seg, variant, int(np.count_nonzero(got != want)))
        ctx.set_variant(0)
        assert plan_tiles(ctx, batch, 0) == plan_tiles(ctx, batch, 1) == 4
        del batch
