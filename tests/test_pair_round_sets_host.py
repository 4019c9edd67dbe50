"""CPU: the sets of tests/pair_round_sets.py have the L, G and M they claim (numpy restatement of the kernel's n_groups,
coordinate bound and owning-lane count), so a sweep's total is the arithmetic's.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import pair_round_sets as S

ROOT = Path(__file__).resolve().parent.parent


def test_the_restated_constants_are_the_kernels():
    csrc = ROOT / "versatiles-glyphs-rs_amd" / "csrc"
    support, kernel = (csrc / "sdf_span_support.h").read_text(), (csrc / "sdf_span_kernel.inc").read_text()
    assert int(re.search(r"constexpr int FCHUNK = (\d+);", support).group(1)) == S.CHUNK
    assert f"constexpr uint32_t GRP = {S.GRP}, NGRP = FCHUNK / GRP;" in kernel
    assert int(re.search(r"constexpr uint32_t QCAP = (\d+);", kernel).group(1)) == S.QCAP
    assert "#define VG_M_SANE(Mc) ((Mc) < 1.0e6f)" in kernel and "#define VG_M_BOUNDED(Mc) ((Mc) < 4096.0f)" in kernel


@pytest.mark.parametrize("total", sorted(S.TOTALS))
def test_far_totals(total):
    L, G = S.TOTALS[total]
    (glyph,) = S.far_total(total)
    segs, _, _, w, h = glyph
    assert S.owning_lanes(w, h) == [L] and S.n_groups(len(segs)) == [G]
    (M,) = S.coord_bounds(glyph)
    assert 4096.0 <= M < 1.0e6
    assert np.array_equal(segs[:, 2:], np.roll(segs[:, :2], -1, axis=0))     # a closed ring
    n = S.far_counters([glyph])
    assert n == {"pairs": total, "rounds": -(-total // 64), "wave_tile_chunks": 1, "pool_overflows": int(total > S.QCAP)}


@pytest.mark.parametrize("name", sorted(S.FAR_SETS))
def test_far_sets_are_unbounded_and_sane(name):
    for glyph in S.FAR_SETS[name]():
        assert all(4096.0 <= M < 1.0e6 for M in S.coord_bounds(glyph)), name


@pytest.mark.parametrize("name", sorted(S.NEAR_SETS))
def test_near_sets_are_bounded(name):
    for glyph in S.NEAR_SETS[name]():
        assert all(M < 4096.0 for M in S.coord_bounds(glyph)), name


def test_what_the_table_reaches():
    tail = {t: (t - 1) % 64 + 1 for t in S.TOTALS}                # entries of a sweep's last round (one pass)
    assert tail[32] == 32 and tail[33] == 33 and tail[96] == 32 and tail[99] == 35 and tail[256] == 64
    passes = {t: -(-t // S.QCAP) for t in S.TOTALS}
    assert passes[256] == 1 and passes[258] == 2 and 258 - S.QCAP == 2 and passes[513] == 3 and 513 - 2 * S.QCAP == 1
    assert passes[2048] == 8 and max(passes.values()) == 8


def test_straddling_lane():
    L, G = S.TOTALS[289]
    assert S.QCAP % G != 0
    lane = S.QCAP // G                                             # its entries G lane .. G lane + G - 1 straddle QCAP
    assert G * lane < S.QCAP < G * (lane + 1) - 1 and lane < L
    (glyph,) = S.straddle()
    first_later = S.QCAP - G * lane                                # the lane's first group in the second window
    assert S.nearest_records(glyph)[lane] // S.GRP >= first_later


def test_winner_in_either_half():
    (glyph,) = S.winner_halves()
    assert len(glyph[0]) == S.GRP and glyph[3] * glyph[4] == 30
    win = set(S.nearest_records(glyph) % S.GRP)
    assert win & {0, 1, 2, 3} and win & {4, 5, 6, 7}


@pytest.mark.parametrize("regime", ["far", "near"])
def test_short_last_groups(regime):
    glyphs = S.short_last_group(regime)
    assert [len(g[0]) - S.GRP for g in glyphs] == [1, 2, 3]
    for g in glyphs:
        assert S.n_groups(len(g[0])) == [2] and S.owning_lanes(g[3], g[4]) == [16]
        near = S.nearest_records(g)
        assert (near >= S.GRP).any() and (near < S.GRP).any()      # either group wins somewhere
    if regime == "far":
        assert S.far_counters(glyphs) == {"pairs": 96, "rounds": 3, "wave_tile_chunks": 3, "pool_overflows": 0}


def test_padding_lanes():
    (g,) = S.padding_lanes()
    assert S.owning_lanes(g[3], g[4]) == [64, 64, 64, 64, 20] and S.n_groups(len(g[0])) == [1]
    assert S.far_counters([g]) == {"pairs": 276, "rounds": 5, "wave_tile_chunks": 5, "pool_overflows": 0}
    (g,) = S.padding_lanes_passes()
    assert S.n_groups(len(g[0])) == [14]
    assert S.far_counters([g]) == {"pairs": 276 * 14, "rounds": 4 * 14 + 5, "wave_tile_chunks": 5, "pool_overflows": 5}


def test_two_chunk_sets():
    for gen, away_chunk in ((S.no_pair_behind, 1), (S.no_pair_first, 0)):
        (g,) = gen()
        segs, x0, y0, w, h = g
        assert len(S.n_groups(len(segs))) == 2 and len(segs) <= 2 * S.CHUNK      # (no chunk-box test up to two chunks)
        far = segs[away_chunk * S.CHUNK:(away_chunk + 1) * S.CHUNK]
        # every end point of the away chunk is farther than 50 px from the window: beyond SAT = 6.2 plus any group radius
        assert min(far[:, 0].min(), far[:, 2].min()) - w > 40 and min(far[:, 1].min(), far[:, 3].min()) - h > 50
