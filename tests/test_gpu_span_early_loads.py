"""GPU: the span kernel's segment loads (csrc/sdf_span_kernel.inc, the stage) bit for bit against the oracle at the edges of
their guard.  Written for a kernel that issues chunk 0's loads as soon as a workgroup has its work-list entry, ahead of the rest
of its prologue; that form was built, passed these cases and was measured slower (profiles/span_startup_ab.txt), so the loads
stay behind the chunk-top barrier.  The cases hold for any issue point:

  segment counts      0 (nothing is loaded), 1, 63 / 64 (a wave), 255 / 256 / 257 (a chunk), 512 / 513 (two chunks; boxes from
                      513), 769 (four chunks, the last of one segment)
  the end of arrays   every count once as the LAST glyph of its batch: its chunk 0 ends where the segment arrays end, and a
                      lane past the count must not load
  a single glyph      every count once as the only glyph
  chunk 0 skipped     a glyph of three chunks whose chunk 0 lies out of reach of every span (loads issued ahead are dropped)
  both layouts        the host's batches (four arrays, stride 1) and a front-end submission (records, stride 4)"""
import numpy as np
import pytest

from test_gpu_span_records import front_end_render, ring, wavy
from test_gpu_span_regimes import CHUNK, WIN, guard_glyph

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 63, 64, 255, 256, 257, 512, 513, 769)
W, H = 24, 40   # 960 px: one span of four tiles, the last tile partial


def counted_glyph(n_seg, k=0):
    """a W x H rect with n_seg segments: a closed ring, or for n_seg = 1 a single slanted segment (an open outline: the bytes
    are whatever the reference's arithmetic gives, which is what the oracle computes)"""
    x0, y0 = k - 3, 2 - k
    if n_seg == 0:
        segs = np.zeros((0, 4))
    elif n_seg == 1:
        segs = np.array([[6.25, 7.5, 17.75, 30.25]])
    else:
        segs = ring(wavy(n_seg, 12.0, 20.0, 8.5, 15.5))
    assert len(segs) == n_seg
    return (segs + [x0, y0, x0, y0], x0, y0, W, H)


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def check(oracle, vg, ctx, glyphs):
    batch = vg.make_batch(glyphs)
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 0)
    ctx.set_variant(0)
    got = ctx.render_batch(batch)
    diff = np.flatnonzero(got != want)
    if diff.size:
        g = int(np.searchsorted(batch.out_off, diff[0], side="right")) - 1
        pytest.fail(f"{diff.size} bytes differ; first: glyph {g} ({batch.seg_off[g + 1] - batch.seg_off[g]} segments), pixel "
                    f"{int(diff[0] - batch.out_off[g])}")


@pytest.mark.parametrize("n_seg", COUNTS)
def test_single_glyph_batches(oracle, vg, ctx, n_seg):
    """the glyph alone: its segments are the whole of the arrays (none at all for n_seg = 0)"""
    check(oracle, vg, ctx, [counted_glyph(n_seg)])


@pytest.mark.parametrize("n_seg", COUNTS)
def test_last_glyph_of_a_batch(oracle, vg, ctx, n_seg):
    """behind the nine other counts: the glyph's chunk 0 (or its last chunk) ends at the end of the segment arrays"""
    others = [counted_glyph(n, k) for k, n in enumerate(COUNTS) if n != n_seg]
    check(oracle, vg, ctx, others + [counted_glyph(n_seg, 5)])


def test_chunk_0_out_of_reach(oracle, vg, ctx):
    """three chunks, so the box test runs; chunk 0 is a ring 50 px above the rect (skipped by every span), chunks 1 and 2 lie in the rect; and the mirror case, the far ring in chunk 2, for the loads behind a processed chunk"""
    first, _ = guard_glyph(("away", "near", "near"), 0.0)
    last, _ = guard_glyph(("near", "near", "away"), 0.0)
    assert len(first) == len(last) == 3 * CHUNK > 2 * CHUNK
    check(oracle, vg, ctx, [(first, 0, 0, WIN, WIN), (last, 0, 0, WIN, WIN)])


def test_counts_through_the_front_end(oracle, vg):
    """closed rings of every count from 3 on as one front-end submission: segment records of 32 bytes (stride 4), entries
    written by outline_plan; in the last glyph a small far ring in front of two near ones makes a chunk 0 that the spans of the
    near rings' rows skip"""
    rings_of = [[wavy(n, 12.0, 20.0, 8.5, 15.5)] for n in COUNTS if n >= 3]
    rings_of.append([wavy(256, 12.0, 90.0, 4.0, 4.0), wavy(256, 12.0, 12.0, 9.0, 9.0), wavy(256, 12.0, 12.0, 6.0, 6.0)[::-1]])
    c = vg.SdfContext(0)
    try:
        front_end_render(oracle, vg, c, rings_of)
        n_seg = np.diff(c.outlines_segments()[0])
        assert [int(n) for n in n_seg[:-1]] == [n for n in COUNTS if n >= 3] and int(n_seg[-1]) == 3 * CHUNK
    finally:
        c.close()
