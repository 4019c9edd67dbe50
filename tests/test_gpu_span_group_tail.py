"""GPU: the span kernel (csrc/sdf_span_kernel.inc) where a chunk's last groups are short or missing, against the oracle (BRUTE
and PRECISE), byte for byte, under both product variants (0: spans, 1: brute force).

The stage's reductions (coordinate bound over a wave, radius over a group's 8 lanes) and the two prefix sums run on DPP steps
whose edge lanes read an identity, and phase 1 reads the 32 group radii four at a time without asking how many groups the
chunk holds.  These are oracle checks of those paths at the shapes where a chunk ends inside a wave, a group or a block of four:

  last chunk of 1, 7, 8, 9, 17, 31, 32, 33, 249, 255, 256 records   n_groups = 1, 1, 1, 2, 3, 4, 4, 5, 32, 32, 32: every residue
                                                                    mod 4, empty groups inside a used block of four, a last
                                                                    group of 1 or 7 records (a radius over fewer than 8 lanes)
  two chunks, 256 + k records                                       chunk 1 holds fewer records and groups than chunk 0: its
                                                                    anchors, radii, coordinate bound and crossing counts must
                                                                    be its own
  windows of 324, 576, 784 and 1600 pixels                          2, 3 and 4 tiles with a partial last one (waves past the end
                                                                    skip the sweep), and two spans
  a vertex 5000 px away                                             Mc >= 4096: `bounded` is false, every real group is a candidate

What they cannot show: a stale or garbage RADIUS in an empty group.  The candidate mask starts as the mask of the chunk's real
groups and the blocks past n_groups carry D_g^2 = 3.4e38, so such a radius never reaches a byte; that the unconditional load is
safe rests on that argument (stated at the load), not on these cases.

Small shapes on purpose: one batch of a few dozen glyphs per test."""
import numpy as np
import pytest

from test_gpu_span_regimes import CHUNK, TILE, coordinate_bound, plan_tiles, ring, run_both, span_count, span_length, spike

pytestmark = pytest.mark.gpu

TAILS = (1, 7, 8, 9, 17, 31, 32, 33, 249, 255, 256)   # records in the last chunk (the issue's list, and 17: three groups)
GRP = 8


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def wobble(n, win, r, reverse=False, phase=0.0):
    """a closed polygon of n >= 3 segments around the middle of a win x win window: radius r with a five-fold ripple, so that the
    groups of 8 consecutive segments differ in radius and no two vertices coincide"""
    a = phase + np.linspace(0, 2 * np.pi, n, endpoint=False)
    c = win / 2.0 + 0.13
    pts = np.stack([c + r * np.cos(a) + 0.045 * win * np.sin(5 * a), c - 0.21 + r * np.sin(a) * 0.93], 1)
    return ring(pts[::-1] if reverse else pts)


def one_chunk(k, win):
    """k records in one chunk (k = 1: a zero-length segment, a closed polygon of one vertex, next to nothing else)"""
    if k == 1:
        p = (win / 2.0 + 0.3, win / 2.0 - 0.4)
        return ring([p])
    if k < 6:
        return wobble(k, win, 0.3 * win)
    inner = max(3, k // 3)
    return np.concatenate([wobble(k - inner, win, 0.36 * win), wobble(inner, win, 0.17 * win, reverse=True, phase=0.4)])


def two_chunks(k, win):
    """256 records in chunk 0 (the outer outline), k in chunk 1 (a hole in the middle; k < 3: the outer outline has 256 + k
    segments and its last k spill over)"""
    if k < 3:
        return wobble(CHUNK + k, win, 0.36 * win)
    return np.concatenate([wobble(CHUNK, win, 0.36 * win), wobble(k, win, 0.15 * win, reverse=True, phase=0.7)])


def groups(n):
    return -(-n // GRP)


assert sorted({groups(k) % 4 for k in TAILS}) == [0, 1, 2, 3] and {k % GRP for k in TAILS} >= {0, 1, 7}   # (module constants)


@pytest.mark.parametrize("win", (24, 40))
def test_last_chunk_tails_in_one_chunk(oracle, vg, ctx, win):
    glyphs = [(one_chunk(k, win), 0, 0, win, win) for k in TAILS]
    assert [len(g[0]) for g in glyphs] == list(TAILS)
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == len(glyphs) * span_count(win, win, 4)


@pytest.mark.parametrize("win", (24, 40))
def test_second_chunk_with_fewer_groups_than_the_first(oracle, vg, ctx, win):
    """256 + k records, k over the listed tails (1, 9 and 33 among them); k = 256: two full chunks, the control"""
    glyphs = [(two_chunks(k, win), 0, 0, win, win) for k in TAILS]
    assert [len(g[0]) - CHUNK for g in glyphs] == list(TAILS)
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert all(span_length(win, len(g[0]), len(glyphs)) == 4 for g in glyphs)


@pytest.mark.parametrize("win,tiles", ((18, 2), (24, 3), (28, 4), (40, 7)))
def test_windows_with_a_partial_last_tile(oracle, vg, ctx, win, tiles):
    """324 px (2 tiles), 576 (3), 784 (4, the last one holding 16 pixels: three of its waves own none) and 1600 (a span of 4 and
    a span of 3), each with short tails in one and in two chunks"""
    assert -(-(win * win) // TILE) == tiles and (win * win) % TILE
    glyphs = [(one_chunk(k, win), 0, 0, win, win) for k in (1, 9, 33, 255)] + [(two_chunks(k, win), 0, 0, win, win) for k in (1, 9, 33)]
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    assert plan_tiles(ctx, batch, 0) == len(glyphs) * span_count(win, win, 4)


def test_tails_where_the_group_bounds_are_off(oracle, vg, ctx):
    """a thin triangle to a vertex 5000 px away puts the chunk's coordinate bound between 4096 and 1e6: the filter is used, the
    group bounds are not, and the candidate mask is the mask of the chunk's real groups alone"""
    win = 24
    far = spike(5000.0)
    glyphs, bounds = [], []
    for k in (7, 9, 33, 255, 256):       # one chunk: the triangle and a ring
        segs = np.concatenate([far, wobble(k - 3, win, 0.3 * win)])
        bounds.append(coordinate_bound(segs))
        glyphs.append((segs, 0, 0, win, win))
    for k in (4, 9, 33):                 # two chunks: chunk 0 bounded, chunk 1 (triangle + a small ring, or the triangle and a spill-over) not
        ring1 = wobble(k - 3, win, 0.15 * win, reverse=True) if k >= 6 else wobble(CHUNK + k - 3, win, 0.36 * win)[CHUNK:]
        head = wobble(CHUNK, win, 0.36 * win) if k >= 6 else wobble(CHUNK + k - 3, win, 0.36 * win)[:CHUNK]
        segs = np.concatenate([head, far, ring1])
        assert len(segs) == CHUNK + k
        assert coordinate_bound(segs[:CHUNK]) < 4096.0
        bounds.append(coordinate_bound(segs[CHUNK:]))
        glyphs.append((segs, 0, 0, win, win))
    assert all(4096.0 <= b < 1.0e6 for b in bounds), bounds
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
