"""GPU: phase 1 of the span kernel (csrc/sdf_span_kernel.inc) at every count of blocks of four groups a chunk can hold,
against the oracle (BRUTE and PRECISE), byte for byte, under both product variants (0: spans, 1: brute force).

Both passes of phase 1 visit only the blocks of four groups the chunk holds (b * 4 < n_groups: scalar branches); the second
pass shifts its reject bits in from the highest real block down to group 0, so a group's bit lands on its own index whatever
the block count is, and the bits above the real blocks are left to the candidate mask.  A full chunk (32 groups) runs the eight
blocks in a straight line; a chunk of 29..31 groups enters the switch at its top (232 records: 29 groups).  A wrong entry
point, a block visited in one pass and not in the other, or a bit off by a multiple of four shows as a missed or a spurious
candidate: a byte.
tests/test_gpu_span_group_tail.py reaches block counts 1, 2 and 8; here every count 1..8 appears, in each place a short chunk
can stand:

  last chunk of 8 (4b - 3) records   the first group of block b alone is real (three empty groups inside a visited block)
  last chunk of 32 b records         block b full
  as a single chunk, as the second chunk behind a full one, as the third of three (the box test is on from three chunks)
  windows of 24 x 24 (one span of 3 tiles) and 40 x 40 (two spans)
  once more at b = 1, 4, 8 with a vertex 5000 px away (`bounded` false: phase 1 is skipped, the mask of real groups alone)

Small shapes on purpose: one batch of 16 glyphs per test."""
import numpy as np
import pytest

from test_gpu_span_group_tail import one_chunk, two_chunks, wobble
from test_gpu_span_regimes import CHUNK, coordinate_bound, plan_tiles, ring, run_both, span_count, span_length, spike  # noqa: F401

pytestmark = pytest.mark.gpu

GRP, BLOCK = 8, 4
BLOCKS = tuple(range(1, 9))
RECORDS = tuple(k for b in BLOCKS for k in (GRP * (BLOCK * b - 3), GRP * BLOCK * b))   # 8, 32, 40, 64, ..., 232, 256


def blocks(k):
    """blocks of four groups the passes visit for a chunk of k records"""
    return -(-(-(-k // GRP)) // BLOCK)


assert sorted({blocks(k) for k in RECORDS}) == list(BLOCKS)                                   # every block count ...
assert all({GRP * (BLOCK * b - 3), GRP * BLOCK * b} <= set(RECORDS) for b in BLOCKS)          # ... first group alone, and full
assert all(blocks(k) == b and -(-k // GRP) in (BLOCK * b - 3, BLOCK * b) for b in BLOCKS for k in RECORDS[2 * b - 2:2 * b])


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def three_chunks(k, win):
    """two full chunks (the outer outline and a second ring inside it), then k records (a hole in the middle)"""
    return np.concatenate([wobble(CHUNK, win, 0.36 * win), wobble(CHUNK, win, 0.27 * win, reverse=True, phase=0.3),
                           wobble(k, win, 0.15 * win, phase=0.7)])


FORMS = {"single_chunk": (one_chunk, 0), "second_chunk": (two_chunks, CHUNK), "third_chunk": (three_chunks, 2 * CHUNK)}


@pytest.mark.parametrize("win", (24, 40))
@pytest.mark.parametrize("form", list(FORMS))
def test_every_block_count(oracle, vg, ctx, form, win):
    make, ahead = FORMS[form]
    glyphs = [(make(k, win), 0, 0, win, win) for k in RECORDS]
    assert [len(g[0]) - ahead for g in glyphs] == list(RECORDS)
    batch = vg.make_batch(glyphs)
    run_both(oracle, vg, ctx, batch, (oracle.BRUTE, oracle.PRECISE))
    T = span_length(win, ahead + 1, len(glyphs))          # (the chunk count decides: 4, 4 and 2 tiles per span)
    assert T == (2 if form == "third_chunk" else 4)
    assert plan_tiles(ctx, batch, 0) == len(glyphs) * span_count(win, win, T)


def test_block_counts_where_the_group_bounds_are_off(oracle, vg, ctx):
    """b = 1, 4 and 8 with a thin triangle to a vertex 5000 px away in the short chunk: its coordinate bound lies between 4096
    and 1e6, so the filter runs over every real group and phase 1 over none"""
    win = 24
    far = spike(5000.0)
    glyphs, bounds = [], []
    for b in (1, 4, 8):
        for k in (GRP * (BLOCK * b - 3), GRP * BLOCK * b):
            tail = np.concatenate([far, wobble(k - 3, win, 0.3 * win)])
            assert len(tail) == k and blocks(k) == b
            glyphs.append((tail, 0, 0, win, win))                                            # one chunk
            bounds.append(coordinate_bound(tail))
            head = wobble(CHUNK, win, 0.36 * win)
            assert coordinate_bound(head) < 4096.0
            small = np.concatenate([far, wobble(k - 3, win, 0.15 * win, reverse=True)])
            glyphs.append((np.concatenate([head, small]), 0, 0, win, win))                   # chunk 0 bounded, chunk 1 not
            bounds.append(coordinate_bound(small))
    assert all(4096.0 <= m < 1.0e6 for m in bounds), bounds
    run_both(oracle, vg, ctx, vg.make_batch(glyphs), (oracle.BRUTE, oracle.PRECISE))
