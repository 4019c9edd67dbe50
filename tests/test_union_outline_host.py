"""CPU: rule U as tests/union_outline_kit.py restates it, against its properties U1 .. U5 and the analytic
yardstick.  No GPU: the device pass is compared with this restatement bit for bit in tests/test_gpu_union_regimes.py.

What rule U changes in the fixture fonts (first 600 code points of the cmap, glyphs with a bitmap): Noto Sans Regular 38 of
596 glyphs rebuilt, 37 bitmaps differ from the reference's; Fira Sans Regular 0 of 597 (every glyph is an identity, U4)."""
import numpy as np
import pytest

import union_outline_kit as K
from conftest import FIRA, NOTO


@pytest.fixture(scope="module")
def noto_glyphs():
    return [(cp, info, segs) + K.union_segments(segs) for cp, info, segs in K.font_glyphs(NOTO, 600)]


@pytest.fixture(scope="module")
def fira_glyphs():
    return [(cp, info, segs) + K.union_segments(segs) for cp, info, segs in K.font_glyphs(FIRA, 600)]


def check_u1_u2_u5(segs, pieces, rect, what):
    x0, y0, w, h = rect
    differing = int((K.winding_nonzero(segs, x0, y0, w, h) != K.winding_nonzero(pieces, x0, y0, w, h)).sum())
    assert differing == 0, f"U1: {what}: {differing} pixel centres change sides"
    assert K.open_points(pieces) == [], f"U2: {what}"
    if len(pieces):   # U5: inside the input's bounding box
        assert pieces[:, [0, 2]].min() >= segs[:, [0, 2]].min() and pieces[:, [0, 2]].max() <= segs[:, [0, 2]].max(), what
        assert pieces[:, [1, 3]].min() >= segs[:, [1, 3]].min() and pieces[:, [1, 3]].max() <= segs[:, [1, 3]].max(), what
        assert not ((pieces[:, 0] == pieces[:, 2]) & (pieces[:, 1] == pieces[:, 3])).any(), what


@pytest.mark.parametrize("name", list(K.RECT_SETS))
def test_rectilinear_sets_equal_the_yardstick(oracle, name):
    """U3: as point sets, and the oracle's raster of both byte for byte (on these coordinates every distance is exact)"""
    segs = K.rect_set_segments(name)
    pieces, _ = K.union_segments(segs)
    yard = K.rect_union_boundary(K.RECT_SETS[name])
    assert K.as_point_set(pieces) == K.as_point_set(yard)
    rect = K.rect_of(segs)
    assert np.array_equal(oracle.sdf_render(pieces, *rect), oracle.sdf_render(yard, *rect))
    assert K.open_points(yard) == []   # (the yardstick's own edges close as well)


@pytest.mark.parametrize("name", list(K.OBLIQUE_SETS))
def test_oblique_sets_equal_their_boundary(oracle, name):
    segs, want = K.OBLIQUE_SETS[name]
    pieces, _ = K.union_segments(segs)
    assert K.as_point_set(pieces) == K.as_point_set(want)
    rect = K.rect_of(segs)
    assert np.array_equal(oracle.sdf_render(pieces, *rect), oracle.sdf_render(want, *rect))


def test_states_and_counts_of_the_exact_sets():
    got = {name: (len(K.union_segments(segs)[0]), K.union_segments(segs)[1]) for name, segs in K.exact_sets().items()}
    assert got["hole"] == (8, K.STATE_IDENTITY) and got["corner_touch"] == (8, K.STATE_IDENTITY)
    assert got["reverse_cancels"] == (0, K.STATE_REBUILT) and got["duplicate"] == (4, K.STATE_REBUILT)
    assert got["nested_same"] == (4, K.STATE_REBUILT) and got["two_rects"] == (8, K.STATE_REBUILT)
    assert got["counter_overlap"] == (12, K.STATE_REBUILT) and got["figure_eight"] == (6, K.STATE_REBUILT)
    # the comb: 70 teeth through the bar; each long edge of the bar is cut 140 times, more than a wave has lanes
    assert got["comb70"] == (4 * 70 + 2 * 70 + 2 + 2 * 71, K.STATE_REBUILT)
    over, st = K.union_segments(K.polygon(12), limit=11)
    assert st == K.STATE_OVER_LIMIT and np.array_equal(over, K.polygon(12))
    bad = K.polygon(12)
    bad[3, 1] = np.nan
    assert K.union_segments(bad)[1] == K.STATE_NON_FINITE


@pytest.mark.parametrize("name", list(K.exact_sets()))
def test_u1_u2_u5_exact_sets(name):
    segs = K.exact_sets()[name]
    check_u1_u2_u5(segs, K.union_segments(segs)[0], K.rect_of(segs), name)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1025])
def test_u1_u2_u5_sized_glyphs(n):
    segs = K.sized_glyph(n)
    assert len(segs) == n
    pieces, st = K.union_segments(segs)
    assert st == K.STATE_REBUILT
    check_u1_u2_u5(segs, pieces, K.rect_of(segs), f"{n} segments")


def test_u1_u2_u5_noto(noto_glyphs):
    for cp, info, segs, pieces, _ in noto_glyphs:
        check_u1_u2_u5(segs, pieces, (info.x0, info.y0, info.w, info.h), f"Noto Sans Regular U+{cp:04X}")


def test_noto_named_glyphs_and_counts(oracle, noto_glyphs):
    by_cp = {g[0]: g for g in noto_glyphs}
    for cp in K.NAMED_NOTO:
        assert by_cp[cp][4] == K.STATE_REBUILT, hex(cp)
    rebuilt = [g for g in noto_glyphs if g[4] == K.STATE_REBUILT]
    assert tuple(g[0] for g in rebuilt) == K.REBUILT_NOTO
    changed = sum(1 for cp, info, segs, pieces, _ in rebuilt
                  if not np.array_equal(oracle.sdf_render(segs, info.x0, info.y0, info.w, info.h),
                                        oracle.sdf_render(pieces, info.x0, info.y0, info.w, info.h)))
    assert (len(noto_glyphs), len(rebuilt), changed) == (596, 38, 37)


def test_u4_fira_is_identity(fira_glyphs):
    """no glyph of Fira's first 600 has a cut point or an interior piece: each comes out as its input less the zero-length
    segments, in input order (and so U1, U2 hold as they do for the input)"""
    assert len(fira_glyphs) == 597
    for cp, info, segs, pieces, st in fira_glyphs:
        assert st == K.STATE_IDENTITY, hex(cp)
        live = segs[~((segs[:, 0] == segs[:, 2]) & (segs[:, 1] == segs[:, 3]))]
        assert pieces.tobytes() == live.tobytes(), hex(cp)
        assert K.open_points(pieces) == [], hex(cp)


def test_the_seam_is_gone(oracle):
    """two overlapping rectangles: every pixel whose centre lies at least 2 px inside the union is saturated over the union's
    segments (>= 254); over the input at least one of them shows the interior edge (<= 210)"""
    rects = K.RECT_SETS["two_rects"]
    segs = K.rect_set_segments("two_rects")
    pieces, _ = K.union_segments(segs)
    x0, y0, w, h = 0, 0, 26, 26
    after = oracle.sdf_render(pieces, x0, y0, w, h)[::-1]   # row 0 = y0
    before = oracle.sdf_render(segs, x0, y0, w, h)[::-1]
    yard = K.rect_union_boundary(rects)   # the analytic boundary: distances to it are exact (axis-parallel edges)
    deep = np.zeros((h, w), dtype=bool)
    for r in range(h):
        for c in range(w):
            px, py = x0 + c + 0.5, y0 + r + 0.5
            inside = any(a <= px <= c2 and b <= py <= d for a, b, c2, d, _ in rects)
            dx = np.maximum(np.maximum(yard[:, [0, 2]].min(axis=1) - px, px - yard[:, [0, 2]].max(axis=1)), 0.0)
            dy = np.maximum(np.maximum(yard[:, [1, 3]].min(axis=1) - py, py - yard[:, [1, 3]].max(axis=1)), 0.0)
            deep[r, c] = inside and np.hypot(dx, dy).min() >= 2.0
    assert deep.sum() >= 10
    assert after[deep].min() >= 255 - 1
    assert before[deep].min() <= 210
