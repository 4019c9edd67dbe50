"""CPU: the directed input sets of tests/raster_margin_sets.py are what they claim to be.  These are conditions on the
INPUTS (no kernel runs here): the expected bytes rest on two independent CPU implementations (the oracle's BRUTE mode
and the numpy restatement of test_numpy_raster_crosscheck.py), every eps tier of every near-boundary set holds at least
one wave's worth of pixels within 2 |eps| of a rounding boundary of the byte, and the undecided-lane sets hold exactly
the number of such pixels per 64-pixel wave of the tile order that their names say."""
import numpy as np
import pytest

import raster_margin_sets as S
from test_numpy_raster_crosscheck import numpy_sdf

NAMES = sorted(S.new_sets())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_numpy_restatement_agree_on_the_set(oracle, vg, name):
    s = S.new_sets()[name]
    batch = vg.make_batch(s.glyphs)
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 4)
    for g, glyph in enumerate(s.glyphs):
        got = numpy_sdf(*glyph).ravel()
        diff = np.flatnonzero(got != want[batch.out_off[g]:batch.out_off[g + 1]])
        assert diff.size == 0, f"{name} glyph {g}: {diff.size} bytes differ, first at {diff[:4]}"


def test_sets_stay_small():
    for name, s in S.new_sets().items():
        assert len(s.glyphs) <= 64, name
        assert sum(len(g[0]) for g in s.glyphs) <= 10000, name
        assert all(g[3] <= 64 and g[4] <= 64 for g in s.glyphs), name


@pytest.mark.parametrize("name", [n for n in NAMES if S.new_sets()[n].near])
def test_every_tier_holds_a_wave_of_near_boundary_pixels(name):
    s = S.new_sets()[name]
    tiers = {}
    for glyph, eps in zip(s.glyphs, s.eps):
        tiers[eps] = tiers.get(eps, 0) + S.witness_count(glyph, eps)
    assert len(tiers) >= 5
    for eps, n in sorted(tiers.items()):
        print(f"{name}: eps 2^{int(np.log2(eps))}: {n} pixels within 2 eps of a boundary")
        assert n >= 64, (name, eps, n)


def test_near_boundary_ladder_and_coordinate_bounds():
    sets = S.new_sets()
    eps = sorted(set(sets["near_boundary"].eps + sets["near_subulp"].eps))
    # from ~1e-3 px down to below the f64 resolution: ulp(32 d + 1/2) = 2^-47 for d in [1, 2) px, i.e. 2^-52 px; the witness
    # of the lowest tiers (|32 d + 1/2 - integer| <= 64 eps, below one ulp) is then a pixel whose f64 value is ON the boundary
    assert eps[-1] >= 2.0 ** -10 and eps[0] <= 2.0 ** -56 and sum(e <= 2.0 ** -52 for e in eps) >= 3
    assert len(eps) >= 16

    def bound(glyph):  # M of the kernel: largest |coordinate| relative to the middle of the bitmap
        segs, x0, y0, w, h = glyph
        return max(np.abs(segs[:, [0, 2]] - (x0 + w // 2)).max(), np.abs(segs[:, [1, 3]] - (y0 + h // 2)).max())

    want = {"near_boundary": (15, 30), "near_subulp": (15, 30), "near_M1e3": (900, 1100), "near_M4000": (3900, 4096), "near_M4200": (4097, 4300),
            "near_M1e6lo": (0.97e6, 1.0e6), "near_M1e6hi": (1.0e6 * 1.00002, 1.03e6)}
    for name, (lo, hi) in want.items():
        for glyph in sets[name].glyphs:
            assert lo <= bound(glyph) < hi, (name, bound(glyph))
    for glyph in sets["abs_position"].glyphs:
        assert glyph[1] >= 2 ** 23 and glyph[1] + glyph[3] <= 2 ** 24 and bound(glyph) < 30
    # pool overflow needs more than 4 groups of 8 records in a chunk whose groups are all candidates (M >= 4096)
    assert all(len(g[0]) > 32 for g in sets["near_M4200"].glyphs)


@pytest.mark.parametrize("name", ["lanes_1", "lanes_2", "lanes_3", "lanes_row"])
def test_undecided_lane_sets_hold_what_they_claim_per_wave(name):
    s = S.new_sets()[name]
    full = 0
    for glyph, eps in zip(s.glyphs, s.eps):
        assert glyph[3] == 64                                    # a wave of the tile order = one row of the bitmap
        counts = S.wave_counts(glyph, eps)
        assert set(counts.tolist()) <= {0, s.per_wave}, (name, counts)
        full += int((counts == s.per_wave).sum())
    assert full >= 16, (name, full)


def test_argmin_pairs_straddle_a_boundary():
    """argmin_swap: for the pixels of the duplicated edges the two candidate distances lie 2^-30 apart, one on either side
    of a rounding boundary (so a kernel that evaluates the wrong one of the two exactly gets another byte)"""
    s = S.new_sets()["argmin_swap"]
    n = 0
    for glyph, eps in zip(s.glyphs, s.eps):
        if eps is None:
            continue
        segs, x0, y0, w, h = glyph
        half = len(segs) // 2
        da, db = S.min_dist(segs[:half], x0, y0, w, h), S.min_dist(segs[half:], x0, y0, w, h)
        sa, sb = 32.0 * da + 0.5, 32.0 * db + 0.5
        n += int(((np.floor(sa) != np.floor(sb)) & (np.abs(sa - sb) < 1e-7)).sum())
    assert n >= 64, n


def test_equality_set_sits_on_the_candidate_rule():
    """cand_equality: for its pixel the far group holds the nearest segment, the candidate rule holds by 2^-16 px in exact
    arithmetic, and the kernel's own f32 form of it FAILS once the inflations are taken away (numpy restatement)"""
    s = S.new_sets()["cand_equality"]
    px, py = S.EQUALITY_PIXEL
    for glyph in s.glyphs:
        segs, x0, y0, w, h = glyph
        d0 = S.min_dist(segs[:8], x0, y0, w, h)[h - 1 - py, px]
        d1 = S.min_dist(segs[8:], x0, y0, w, h)[h - 1 - py, px]
        assert 0.5 * S.EQUALITY_DELTA < d1 - d0 < 2 * S.EQUALITY_DELTA                        # group 0 is nearer, by delta
        assert np.floor(32.0 * d0 + 0.5) + 1 == np.floor(32.0 * d1 + 0.5)                     # and gives another byte
        a_g, p = segs[4, :2], np.array([x0 + px + 0.5, y0 + py + 0.5])
        slack = d1 + np.hypot(*(segs[4, 2:] - a_g)) - np.hypot(*(p - a_g))                     # U + r_g - D_g, f64
        assert 0 < slack < 2 * S.EQUALITY_DELTA
        res = S.phase1_residuals(glyph, (px, py))
        assert res[0] < 0 < res[1], res
