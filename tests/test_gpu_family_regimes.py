"""The upload kernels of submissions that name code-point ranges of resident families (family_expand / family_gather,
csrc/family_upload_kernel.inc) at their edges: 256 glyphs per workgroup, tasks that begin and end on, before and behind a
workgroup's boundary, many tasks inside one workgroup and one task over three, tasks that map nothing, ranges that cut a block
at its first and last code point, repeated / overlapping / descending tasks, glyph ids without outline where a task's reserved
room goes, the 128 font references a workgroup keeps in LDS, families that share a font, very large glyphs, and the
context-pass route of a family with an odd scale.

The fonts are synthetic (the command fonts of test_gpu_resident_gather_regimes.py, the composite glyf fonts of
test_gpu_resident_expand_regimes.py).  The yardstick is vgsdf_outlines_submit_resident of the glyph sequence the ranges stand
for — rects, sizes, every segment bit for bit, every bitmap, the positions of the in-place PBF arena — through
tests/test_gpu_resident_fonts.py's _assert_same; both kinds of font, with and without pbf_pre.  No tolerance appears anywhere.
"""
import numpy as np
import pytest

import family_ranges_kit as K
from family_ranges_kit import GROUP, compare, random_family

pytestmark = pytest.mark.gpu

KINDS = ["commands", "glyf"]


@pytest.fixture(params=KINDS)
def kit(vg, request):
    ctx = vg.SdfContext(0)
    try:
        yield K.make_kit(vg, ctx, request.param)
    finally:
        ctx.close()


def span(fam, i, count, pre=0, k=0):
    """the task of family k over exactly its entries [i, i + count)"""
    return (k, int(fam.cp[i]), int(fam.cp[i + count - 1]), pre)


def test_the_restated_constants_are_the_kernels(vg):
    import ctypes as C
    cache = C.c_uint32()
    vg.load_library().vgsdf_glyf_limits(None, None, C.byref(cache))
    assert cache.value == K.FONT_CACHE


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_one_task_of_n_glyphs(kit, n):
    fam = random_family(kit, n, 300)
    rects = compare(kit.ctx, [fam], [span(fam, 7, n, pre=19)])
    assert len(rects) == n and int(rects["has_raster"].sum()) == n
    assert fam.handle.count(int(fam.cp[7]), int(fam.cp[7 + n - 1])) == n and fam.handle.device_bytes >= 27 * 300 + 8 * 301


def test_task_boundaries_around_the_workgroup_size(kit):
    """tasks that end on, one before and one behind every multiple of 256 glyphs, in one submission and one by one"""
    fam = random_family(kit, 11, 900)
    sizes = [255, 1, 1, 255, 1, 256, 257, 254, 1, 2, 253]      # boundaries at 255 256 257 | 512 513 | 769 | 1026 1280 1281 1283 1536
    ends = np.cumsum(sizes)
    assert {255, 256, 257, 512, 513, 1280, 1281, 1536} <= set(int(e) for e in ends)
    tasks, at = [], 0
    for j, s in enumerate(sizes):
        tasks.append(span(fam, at % 600, s, pre=10 + j))
        at += 97
    rects = compare(kit.ctx, [fam], tasks)
    assert len(rects) == ends[-1]
    for cut in (255, 256, 257):                                    # two tasks whose boundary falls there
        compare(kit.ctx, [fam], [span(fam, 0, cut, pre=5), span(fam, 300, 300, pre=6)])


def test_300_one_glyph_tasks(kit):
    """more tasks than lanes in one workgroup's reach: every lane its own task, and a workgroup that begins in the middle of them"""
    fam = random_family(kit, 5, 400)
    order = np.random.default_rng(1).permutation(300)
    rects = compare(kit.ctx, [fam], [span(fam, int(i), 1, pre=int(i) % 40) for i in order])
    assert len(rects) == 300


def test_one_task_over_three_workgroups(kit):
    fam = random_family(kit, 6, 800)
    rects = compare(kit.ctx, [fam], [span(fam, 50, 700, pre=33)])
    assert len(rects) == 700 > 2 * GROUP


def test_tasks_that_map_nothing(kit):
    """first, last, between the others and side by side; alone; and no task at all.  Their extents are empty (compare)"""
    fam = random_family(kit, 8, 300, first_cp=1000, gaps=(2, 3))
    hole = int(next(c for c in range(1001, 3000) if c not in set(fam.cp.tolist())))
    nothing = [(0, 0, 999, 9), (0, hole, hole, 11), (0, int(fam.cp[-1]) + 1, 0xFFFF, 13)]
    full = [span(fam, 3, 40, pre=21), span(fam, 100, 200, pre=22)]
    for tasks in ([nothing[0]] + full, full + [nothing[2]], [full[0], nothing[1], full[1]], [nothing[0], nothing[1], full[0], nothing[2], nothing[0], full[1], nothing[1]]):
        rects = compare(kit.ctx, [fam], tasks)
        assert len(rects) == 240
    for tasks in ([nothing[1]], nothing, []):
        assert len(compare(kit.ctx, [fam], tasks)) == 0
    # the context renders on
    assert len(compare(kit.ctx, [fam], full[:1], layouts=(True,))) == 40


def test_ranges_that_cut_a_block(kit):
    """256-aligned blocks of code points: a range that is the block, ranges that begin / end exactly on the block's first and
    last mapped code point and one off either, ranges wider than a block and the whole of the code points"""
    fam = random_family(kit, 9, 700, first_cp=250, gaps=(1, 2))
    cp = fam.cp
    lo, hi = 512, 767
    inside = cp[(cp >= lo) & (cp <= hi)]
    a, b = int(inside[0]), int(inside[-1])
    tasks = [(0, lo, hi, 24), (0, a, b, 24), (0, a + 1, b, 3), (0, a, b - 1, 4), (0, a - 1, b + 1, 5), (0, a, a, 6), (0, b, b, 7),
             (0, lo - 300, hi + 300, 8), (0, 0, 0xFFFF, 9), (0, 256, 511, 24), (0, 768, 1023, 24)]
    rects = compare(kit.ctx, [fam], tasks)
    assert len(rects) == sum(fam.handle.count(t[1], t[2]) for t in tasks) > 3 * GROUP


def test_repeated_overlapping_and_descending_tasks(kit):
    fam = random_family(kit, 10, 500)
    t = span(fam, 20, 90, pre=17)
    tasks = [t, t, t, span(fam, 60, 100, pre=1), span(fam, 100, 30, pre=2), span(fam, 0, 500, pre=3)]
    compare(kit.ctx, [fam], tasks)
    compare(kit.ctx, [fam], [span(fam, 400 - 40 * j, 40, pre=j) for j in range(10)])       # descending code points


def test_glyph_ids_without_outline_open_and_close_a_task(kit):
    """pbf_pre lands on a glyph without a raster; so does the end of a task, of a workgroup and of the submission"""
    empty_at = [10, 49, 50, 99, 100, 100 + GROUP - 1, 100 + GROUP, 399]
    fam = random_family(kit, 12, 400, empty_at=empty_at)
    tasks = [span(fam, 10, 40, pre=23), span(fam, 50, 50, pre=24), span(fam, 100, 300, pre=25), span(fam, 399, 1, pre=26), span(fam, 49, 2, pre=0)]
    rects = compare(kit.ctx, [fam], tasks)
    firsts = np.cumsum([0] + [fam.handle.count(t[1], t[2]) for t in tasks])[:-1]
    assert (rects["has_raster"][firsts] == 0).all() and (rects["has_raster"][firsts[1:] - 1] == 0).all() and rects["has_raster"][-1] == 0
    assert int(rects["has_raster"].sum()) == len(rects) - 11


@pytest.mark.parametrize("n_fonts", [1, 128, 129, 200])
def test_families_around_the_font_cache(kit, n_fonts):
    """a family over n_fonts fonts (the three handles again and again: neighbours differ), and a second family behind it whose
    fonts begin at n_fonts in the block's list — either side of the 128 references a workgroup keeps in LDS"""
    font_list = [i % len(kit.kinds) for i in range(n_fonts)]
    a = random_family(kit, n_fonts, 600, font_list=font_list)
    b = random_family(kit, n_fonts + 1, 100, font_list=[2, 0])
    assert set(a.font_of.tolist()) == set(range(n_fonts))
    tasks = [span(a, 0, 600, pre=9), span(b, 0, 100, pre=8, k=1), span(a, 300, 10, pre=7), span(b, 50, 50, pre=6, k=1)]
    compare(kit.ctx, [a, b], tasks)
    compare(kit.ctx, [b, a], [(1 - k, f, l, p) for k, f, l, p in tasks], layouts=(True,))


def test_two_families_share_a_font(kit):
    a = random_family(kit, 20, 200, font_list=[0, 1])
    b = random_family(kit, 21, 200, font_list=[1, 2], first_cp=40)
    tasks = [span(a, 0, 150, pre=4), span(b, 10, 150, pre=5, k=1), span(a, 150, 50, pre=6), span(b, 0, 10, pre=7, k=1)]
    compare(kit.ctx, [a, b], tasks)
    # one family listed twice is two families of the block
    compare(kit.ctx, [a, a], [span(a, 0, 20, pre=4), span(a, 5, 20, pre=5, k=1)], layouts=(True,))


def test_a_very_large_glyph(kit):
    """5000 commands (command fonts: more than a workgroup gathers in a round) / 600 leaves (glyf fonts: more than a workgroup has
    lanes): alone, first and last of a task, last glyph of a workgroup and first of the next"""
    big_at = [0, 30, 59, 60, 60 + GROUP - 1, 60 + GROUP]
    fam = random_family(kit, 13, 400, big_at=big_at)
    compare(kit.ctx, [fam], [span(fam, 0, 1, pre=12)])
    compare(kit.ctx, [fam], [span(fam, 30, 30, pre=12), span(fam, 60, 340, pre=13)])


def test_a_family_with_an_odd_scale_takes_the_context_pass(kit):
    """one scale that is not positive and finite in the family: no submission against it trusts the gathered / decoded context
    bytes, whether or not its ranges reach that entry"""
    for odd in (-0.02, np.inf, np.nan):
        fam = random_family(kit, 14, 300, odd_scale=(120, odd), empty_at=[] if odd == -0.02 else [120])
        compare(kit.ctx, [fam], [span(fam, 100, 50, pre=3), span(fam, 0, 40, pre=4)], layouts=(True,) if odd != -0.02 else (False, True))
        compare(kit.ctx, [fam], [span(fam, 0, 100, pre=3)], layouts=(False,))


def test_the_upload_depends_on_tasks_fonts_and_families_alone(kit):
    """(compare asserts 32 bytes per task that maps a glyph, family and font on every submission) the same tasks over ranges of
    10 and of 500 glyphs upload the same block"""
    fam = random_family(kit, 15, 600, font_list=[0, 1, 2])
    for count in (10, 500):
        compare(kit.ctx, [fam], [span(fam, 0, count), span(fam, 50, count)], layouts=(False,))
        assert kit.ctx.resident_upload_bytes() == 32 * (2 + 1 + 3)


def test_more_families_than_a_workgroup_keeps_in_lds(kit):
    """70 families in one block: the records of the first 64 (kFamilyCache) are read from LDS, the others from the block"""
    fams = [random_family(kit, 30 + k, 40, font_list=[k % 3], first_cp=10 + k) for k in range(70)]
    tasks = [span(fams[k], (3 * k) % 20, 20, pre=k, k=k) for k in (0, 1, 62, 63, 64, 65, 69, 63, 64, 0, 69)]
    rects = compare(kit.ctx, fams, tasks)
    assert len(rects) == 220
    compare(kit.ctx, fams, [span(fams[k], 0, 40, pre=1, k=k) for k in range(70)], layouts=(True,))
