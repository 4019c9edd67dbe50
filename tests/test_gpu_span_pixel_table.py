"""GPU: the span kernel's per-pixel coordinate table and its pooled pair entries (csrc/sdf_span_kernel.inc, pix_pack in
csrc/sdf_span_support.h), against the oracle (BRUTE and PRECISE), byte for byte, under both product variants (0: spans, 1:
brute force).

The kernel divides a pixel's column and row out once per workgroup and keeps them in 4 bytes of LDS (f16 column offset from
the bitmap's middle, 16-bit row offset inside the span); every sweep (one per chunk), the exact evaluations and the final
stores read that entry.  A pooled (pixel, group) pair is stored as its two LDS byte offsets (lane * 4 and group * 32).

  widths 1, 2, 3, 31, 63, 64, 65, 255, 256, 257, 1022     the f16's range (|rpx| <= 511.5 at w = 1022) and its parity (w >> 1),
                                                          odd and even heights, one chunk and 2-3 chunks (later chunks read
                                                          the table; three chunks turn the box test on)
  w = 1 and 3 at h = 2100                                 row index beyond 2047, row offset inside the span small
  x0, y0 negative and at +-2^23                           the integer column / row rebuilt from the entry for the f64
                                                          evaluation (a large |x0| makes many pixels take it)
  T = 1, 2, 3, 4 x a last tile of 1, 64, 65, 255 pixels   padding lanes (entry of the bitmap's last pixel, candidate mask cleared)
  a 256-segment ring, start vertex rotated 32 times      every group index nearest to pixels of every lane quarter: the
                                                          entry's fields at lane 63 and group 31
  three dense shapes                                      waves without a pair, a pool overflow, no overflow; the counting
                                                          instance of the margins build (vgsdf_set_variant 61) is the witness

Small shapes on purpose: a few dozen glyphs per batch, bitmaps of at most ~4000 pixels (6300 at h = 2100)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_span_group_tail import wobble
from test_gpu_span_regimes import CHUNK, TILE, plan_tiles, ring, run_both, span_count, span_length

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MARGINS_LIB = ROOT / "versatiles-glyphs-rs_amd" / "build" / "margins" / "libvgsdf.so"


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def outline(w, h, n_seg):
    """n_seg segments for a w x h window at (0, 0): rippled ellipses around its middle, 256 per ring (the last one shorter), so
    that ring i is chunk i; vertices off the pixel centres"""
    cx, cy = w / 2.0 + 0.13, h / 2.0 - 0.21
    rings, left, i = [], n_seg, 0
    while left > 0:
        n = min(left, CHUNK)
        assert n >= 3
        a = 0.3 * i + np.linspace(0, 2 * np.pi, n, endpoint=False)
        f = 0.40 - 0.11 * i
        pts = np.stack([cx + (f * w + 0.4) * np.cos(a) + 0.03 * w * np.sin(5 * a), cy + (f * h + 0.4) * np.sin(a)], 1)
        rings.append(ring(pts[::-1] if i % 2 else pts))
        left -= n
        i += 1
    return np.concatenate(rings)


def glyph(w, h, n_seg, x0=0, y0=0):
    segs = outline(w, h, n_seg)
    segs[:, [0, 2]] += x0
    segs[:, [1, 3]] += y0
    return (segs, x0, y0, w, h)


def expected_spans(glyphs):
    return sum(span_count(w, h, span_length(w, len(s), len(glyphs))) for s, _, _, w, h in glyphs)


# (w, h): every listed width with an odd and an even height, w * h below ~4000
WINDOWS = ((1, 37), (1, 300), (2, 51), (2, 50), (3, 41), (3, 40), (31, 31), (31, 30), (63, 33), (63, 32), (64, 33), (64, 32),
           (65, 31), (65, 30), (255, 15), (255, 14), (256, 15), (256, 14), (257, 13), (257, 12), (1022, 3), (1022, 2))
assert {w for w, _ in WINDOWS} == {1, 2, 3, 31, 63, 64, 65, 255, 256, 257, 1022}
assert all({h % 2 for ww, h in WINDOWS if ww == w} == {0, 1} for w, _ in WINDOWS) and max(w * h for w, h in WINDOWS) < 4000


@pytest.mark.parametrize("n_seg", (40, 300, 600), ids=lambda n: f"{-(-n // CHUNK)}chunk")
def test_window_widths(oracle, vg, ctx, n_seg):
    glyphs = [glyph(w, h, n_seg) for w, h in WINDOWS]
    assert all(len(g[0]) == n_seg for g in glyphs)
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == expected_spans(glyphs)


def test_rows_beyond_2047(oracle, vg, ctx):
    """w = 1 (spans of 2 tiles = 512 rows) and w = 3 at h = 2100: the last spans start beyond row 2047, and a span's row offset
    stays below 512; one chunk and two"""
    glyphs = [glyph(w, 2100, n) for w in (1, 3) for n in (40, 300)]
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == expected_spans(glyphs)
    assert span_length(1, 40, 4) == 2 and (2100 - 1) // (2 * TILE) * 2 * TILE > 2047


def test_origins(oracle, vg, ctx):
    """x0, y0 negative and at +-2^23, odd and even widths; the ring's vertices keep their fractions (exact in f64 at 2^23)"""
    big = 2 ** 23
    glyphs = []
    for x0, y0 in ((-7, -11), (-big, -big), (big, big), (-big, big), (big, -3), (-5, -big)):
        for w, h in ((31, 30), (64, 33), (255, 15)):
            for n in (40, 300):
                glyphs.append(glyph(w, h, n, x0, y0))
    batch = vg.make_batch(glyphs)
    assert int(batch.x0.min()) == -big and int(batch.y0.max()) == big
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == expected_spans(glyphs)


def last_span_window(T, r):
    """(w, h) of the smallest bitmap of 1024 m + 256 (T - 1) + r pixels (m = 0 .. 3) whose width takes spans of 4 tiles: its last
    span has T tiles and the last of them r pixels"""
    for m in range(4):
        n = 1024 * m + TILE * (T - 1) + r
        for w in range(3, 511):
            if n % w == 0 and span_length(w, 40) == 4:
                return w, n // w
    raise AssertionError((T, r))


LAST_TILES = [(T, r) + last_span_window(T, r) for T in (1, 2, 3, 4) for r in (1, 64, 65, 255)]


def test_last_tiles(oracle, vg, ctx):
    """the last span's length and the last tile's pixel count crossed: 1 pixel (one lane of one wave), 64 (one wave exactly), 65
    and 255 (one lane short of the tile)"""
    glyphs = []
    for T, r, w, h in LAST_TILES:
        assert (w * h) % 1024 == TILE * (T - 1) + r and -(-((w * h) % 1024) // TILE) == T
        glyphs += [glyph(w, h, 40), glyph(w, h, 300)]
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == expected_spans(glyphs)


def test_rotated_start_vertex(oracle, vg, ctx):
    """a ring of 256 segments in a 24 x 24 window (3 tiles: 9 waves with pixels), its start vertex rotated by one group 32
    times: group g of rotation r is the arc that group (g + r) % 32 was, so every group index, 31 included, comes nearest to
    the pixels of every wave and lane, 63 included"""
    win = 24
    base = wobble(CHUNK, win, 0.36 * win)
    glyphs = [(np.roll(base, -8 * r, axis=0), 0, 0, win, win) for r in range(32)]
    assert all(np.array_equal(g[0][:, 2:], np.roll(g[0][:, :2], -1, axis=0)) for g in glyphs)     # still closed rings
    batch = vg.make_batch(glyphs)
    want = run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    px = win * win
    assert all(np.array_equal(want[:px], want[r * px:(r + 1) * px]) for r in range(32))             # the same picture 32 times


# ---------------------------------------------------------------------------------------------------------------------
# the pair pool at its regimes
# ---------------------------------------------------------------------------------------------------------------------

def dense_shapes():
    """three shapes of 256 short segments:
    corner   a ring of radius 2.5 px in the corner of a 40 x 40 window: the waves farther than the saturation distance hold no pair
    blob     32 laps of an octagon of radius 1.2 px in the middle of an 8 x 8 window: every group is the same octagon, so all 32
             are candidates of all 64 pixels (2048 pairs against a pool of 256: every pixel walks its own list)
    wide     a ring of radius 23 px in a 64 x 64 window (a wave = one row): a pixel meets at most a handful of groups"""
    a = np.linspace(0, 2 * np.pi, CHUNK, endpoint=False)
    corner = ring(np.stack([4.3 + 2.5 * np.cos(a), 35.2 + 2.5 * np.sin(a)], 1))
    o = np.linspace(0, 2 * np.pi, 8, endpoint=False)
    blob = ring(np.tile(np.stack([4.1 + 1.2 * np.cos(o), 3.8 + 1.2 * np.sin(o)], 1), (32, 1)))
    wide = ring(np.stack([32.2 + 23.0 * np.cos(a) + 1.5 * np.sin(5 * a), 31.7 + 23.0 * np.sin(a)], 1))
    return {"corner": (corner, 0, 0, 40, 40), "blob": (blob, 0, 0, 8, 8), "wide": (wide, 0, 0, 64, 64)}


COUNT_CHILD = r'''
import ctypes, json, sys
sys.path.insert(0, "tests")
from conftest import load_product
import test_gpu_span_pixel_table as P
vg = load_product()
lib = vg.load_library()
lib.vgsdf_margin_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
lib.vgsdf_margin_counters.restype = ctypes.c_int
c = vg.SdfContext(0)
c.set_variant(61)
doc = {}
for name, g in P.dense_shapes().items():
    assert lib.vgsdf_margin_counters(None, 1) == 0
    out = c.render_batch(vg.make_batch([g]))
    n = (ctypes.c_ulonglong * 9)()
    assert lib.vgsdf_margin_counters(n, 0) == 0
    doc[name] = {"pairs": int(n[1]), "rounds": int(n[2]), "wave_tile_chunks": int(n[3]), "pool_overflows": int(n[6]),
                 "bytes": out.tobytes().hex()}
c.close()
print(json.dumps(doc))
'''


def test_pair_pool_regimes(oracle, vg, ctx):
    shapes = dense_shapes()
    want = {}
    for name, g in shapes.items():
        want[name] = run_both(oracle, vg, ctx, vg.make_batch([g]), (oracle.BRUTE, oracle.PRECISE))
    if not MARGINS_LIB.exists():
        pytest.skip("bytes checked; the counters need the margins build (make -C versatiles-glyphs-rs_amd margins)")
    cp = subprocess.run([sys.executable, "-c", COUNT_CHILD], cwd=ROOT, env=dict(os.environ, VGSDF_LIB=str(MARGINS_LIB)),
                        capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-3000:]
    doc = json.loads(cp.stdout.strip().splitlines()[-1])
    for name in shapes:                                     # the counting instance renders the same bytes
        assert bytes.fromhex(doc[name]["bytes"]) == want[name].tobytes(), name
    n = {k: {c: v for c, v in d.items() if c != "bytes"} for k, d in doc.items()}
    # waves with pixels x chunks: 25 of the 40 x 40 window, 1 of the 8 x 8, 64 of the 64 x 64
    assert [n[k]["wave_tile_chunks"] for k in ("corner", "blob", "wide")] == [25, 1, 64], n
    # corner: a wave with a pair takes at least one round, so fewer rounds than waves means waves whose total is 0
    assert 0 < n["corner"]["rounds"] < n["corner"]["wave_tile_chunks"] and n["corner"]["pairs"] > 0, n
    # blob: 64 pixels x 32 groups, over the pool's 256
    assert n["blob"] == {"pairs": 2048, "rounds": 32, "wave_tile_chunks": 1, "pool_overflows": 1}, n
    # wide: every wave inside the pool
    assert n["wide"]["pool_overflows"] == 0 and n["wide"]["pairs"] > 0, n
