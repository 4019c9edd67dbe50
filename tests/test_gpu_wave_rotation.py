"""GPU: the span kernel's rotation of a tile's pixels over the four waves (rot, a hash of the workgroup's index: thread tid
owns pixel p0 + k 256 + ((tid + 64 rot) & 255) in the sweep and in the final stores), bit-exact against the oracle (PRECISE
and BRUTE).

Synthetic glyphs whose pixel counts hit every remainder of the 64-pixel quarters and of the 256-pixel tiles and every span
length, with 8, 256, 257 and 600 segments (1, 2 and 3 chunks; the last takes the chunk-box test), and one glyph without
segments per shape (the zeroed histogram and the neutral bytes).  Every glyph is in the batch 64 times: its copies take
consecutive positions of the work list, so every rot value and every XCD residue meets every shape (checked on the restated
work list of tools/model_wave_shares.py), and all copies must give the same bytes.

  host plan     ctx.upload / launch / download under variant 0: all shapes
  device plan   the same rings as command streams through outlines_prepare / outlines_render (the launch behind the plan's
                guard).  The front-end makes its own rects, bounding box + 3 px on every side, so w, h >= 7: the 1 x 1, 65 px
                and 257 px shapes (1 x 1, 13 x 5, 257 x 1) and the glyphs without segments (no raster) are the host plan's only."""
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_front_end_regimes import _stream

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

COPIES = 64
SEGMENTS = (8, 256, 257, 600)
# (w, h): 1, 63, 64, 65, 256, 257, 272, 1023, 1024, 1025 px, and w = 70 (a histogram row longer than one wave; 1400 px)
SHAPES = ((1, 1), (9, 7), (8, 8), (13, 5), (16, 16), (257, 1), (17, 16), (33, 31), (32, 32), (41, 25), (70, 20))
PIXELS = (1, 63, 64, 65, 256, 257, 272, 1023, 1024, 1025, 1400)


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def outline(w, h, n_seg):
    """one ring of n_seg distinct points on a wobbly ellipse, on multiples of 1/4096 px (exact in the front-end's f32 commands); for
    w, h >= 7 its bounding box is exactly [0.25, w - 6.25] x [0.25, h - 6.25], so that the front-end's rect (floor / ceil + 3 px)
    is (-3, -3, w, h); smaller rects show a part of a ring of 4 x 3 px at their corner"""
    a = np.linspace(0, 2 * np.pi, n_seg, endpoint=False) + 0.1
    r = 1 + 0.2 * np.sin(5 * a + w)
    ex, ey = (w - 6.5, h - 6.5) if w >= 7 and h >= 7 else (4.0, 3.0)
    x, y = r * np.cos(a), r * np.sin(a)
    x = 0.25 + (x - x.min()) / (x.max() - x.min()) * ex
    y = 0.25 + (y - y.min()) / (y.max() - y.min()) * ey
    pts = np.round(np.stack([x, y], 1) * 4096) / 4096
    for col, ext in ((0, ex), (1, ey)):   # the extremes exactly on the box (rounding kept them within 1/8192 of it)
        pts[np.argmin(pts[:, col]), col] = 0.25
        pts[np.argmax(pts[:, col]), col] = 0.25 + ext
    return pts


def unique_glyphs():
    """[(segs, x0, y0, w, h)]: every shape with every segment count, then every shape without segments"""
    out = []
    for w, h in SHAPES:
        for n_seg in SEGMENTS:
            out.append((ring(outline(w, h, n_seg)), -3, -3, w, h))
    for w, h in SHAPES:
        out.append((np.zeros((0, 4)), -3, -3, w, h))
    return out


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected(oracle, vg):
    """the unique glyphs and the oracle's bytes of each (both modes agree), computed once"""
    glyphs = unique_glyphs()
    batch = vg.make_batch(glyphs)
    want, _ = oracle.sdf_render_batch(batch, oracle.PRECISE, 0)
    brute, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 0)
    assert np.array_equal(want, brute), "the oracle's modes disagree"
    return glyphs, [want[a:b] for a, b in zip(batch.out_off[:-1], batch.out_off[1:])]


def first_difference(got, want_of, copies):
    """got: the bytes of every glyph `copies` times in a row -> None, or (unique glyph, copy, pixel, got, want) of the first wrong byte"""
    off = 0
    for u, want in enumerate(want_of):
        for c in range(copies):
            mine = got[off:off + len(want)]
            if not np.array_equal(mine, want):
                p = int(np.flatnonzero(mine != want)[0])
                return u, c, p, int(mine[p]), int(want[p])
            off += len(want)
    assert off == len(got)
    return None


def test_the_shapes_are_the_intended_ones(expected):
    glyphs, want_of = expected
    assert tuple(w * h for w, h in SHAPES) == PIXELS
    assert [len(g[0]) for g in glyphs[:len(SEGMENTS)]] == list(SEGMENTS)
    for g, want in zip(glyphs, want_of):
        assert len(want) == g[3] * g[4]
        assert np.all((g[0][:, :2] != g[0][:, 2:]).any(axis=1))    # no segment of length zero (the front-end would drop it)
        assert np.array_equal(g[0], g[0].astype(np.float32))
        if len(g[0]) == 0:
            assert not want.any()          # no segment: every pixel is outside and saturated
        elif g[3] >= 7 and g[4] >= 7:
            assert want.max() > 191        # the ring is inside the rect: some pixel is inside it


def test_every_rotation_and_xcd_meets_every_shape(expected):
    """the restated work list (tools/model_wave_shares.py: the host planner's order and the kernel's hash): the workgroups of
    the 64 copies of every glyph take all four rot values and all eight XCD residues"""
    sys.path.insert(0, str(ROOT / "tools"))
    import model_wave_shares as M
    glyphs, _ = expected
    w = np.repeat([g[3] for g in glyphs], COPIES)
    h = np.repeat([g[4] for g in glyphs], COPIES)
    n_seg = np.repeat([len(g[0]) for g in glyphs], COPIES)
    seen = {}
    for b, (g, p, _) in enumerate(M.work_list(w, h, n_seg)):
        seen.setdefault((g // COPIES, p), set()).add((M.wave_rot(b), b % 8))
    assert len(seen) == len(glyphs) + 2 * (len(SEGMENTS) + 1)    # one span each; two for the 1025 px and the 1400 px shapes
    assert all(len({r for r, _ in s}) == 4 and len({x for _, x in s}) == 8 for s in seen.values())


def test_host_plan_variant_0(vg, ctx, expected):
    glyphs, want_of = expected
    batch = vg.make_batch([g for g in glyphs for _ in range(COPIES)])
    ctx.set_variant(0)
    db = ctx.upload(batch)
    try:
        db.launch()
        got = db.download()
        n_tiles = db.stats()["n_tiles"]
    finally:
        db.free()
    assert n_tiles == COPIES * (len(glyphs) + 2 * (len(SEGMENTS) + 1))
    bad = first_difference(got, want_of, COPIES)
    assert bad is None, f"(unique glyph, copy, pixel, got, want) = {bad}; glyph: w, h = {glyphs[bad[0]][3:]}, {len(glyphs[bad[0]][0])} segments"


def test_device_plan(oracle, vg, expected):
    glyphs, want_of = expected
    mine = [(u, g) for u, g in enumerate(glyphs) if len(g[0]) and g[3] >= 7 and g[4] >= 7]
    assert sorted({g[3] * g[4] for _, g in mine}) == [63, 64, 256, 272, 1023, 1024, 1025, 1400]
    parts, lens = [], []
    for _, g in mine:
        st = _stream([g[0][:, :2]], 1.0)
        one = np.array([(c[1], c[2], c[3], c[4], c[5], c[6], c[0]) for c in st], dtype=vg.OUTLINE_CMD_DTYPE)
        parts += [one] * COPIES
        lens += [len(one)] * COPIES
    cmd_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n = len(lens)
    c = vg.SdfContext(0)
    try:
        rects, ob, ns = c.outlines_prepare(cmd_off, np.concatenate(parts), np.ones(n), np.zeros(n))
        out = c.outlines_render()
        seg_off, segs = c.outlines_segments()
    finally:
        c.close()
    for k, (_, g) in enumerate(mine):      # the front-end made the intended rects and segments: the oracle's bytes apply
        r = rects[k * COPIES]
        assert (int(r["has_raster"]), int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])) == (1, -3, -3, g[3], g[4]), k
        a = k * COPIES
        assert segs[seg_off[a]:seg_off[a + 1]].tobytes() == g[0].tobytes(), k
    assert ns == COPIES * sum(len(g[0]) for _, g in mine) and ob == len(out) == COPIES * sum(g[3] * g[4] for _, g in mine)
    bad = first_difference(out, [want_of[u] for u, _ in mine], COPIES)
    assert bad is None, f"(glyph of the device set, copy, pixel, got, want) = {bad}"
