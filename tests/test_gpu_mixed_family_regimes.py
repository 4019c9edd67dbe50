"""Ranges submissions over MIXED families (vgsdf_family_create_mixed; family_mixed, the third stamping of
csrc/family_upload_kernel.inc) at their edges: entries whose fonts alternate in kind, tasks that straddle workgroups, tasks of one
glyph, two mixed families in one submission, repeated and overlapping tasks, a mixed family whose fonts are all of one kind, tasks
that map nothing, very large glyphs of both kinds, the font cache with both kinds on either side, and the refusal of a mixed family
beside a family of one kind.

The fonts are synthetic (tests/mixed_kinds_kit.py).  The yardstick is vgsdf_outlines_submit_resident_mixed of the glyph sequence the
ranges stand for (pinned to the single-kind calls by tests/test_gpu_mixed_named_regimes.py) — rects, sizes, every segment bit for
bit, every bitmap, the positions of the in-place PBF arena, the upload's 32 bytes per live task, family and font, the tasks'
extents — as family_ranges_kit.compare does for families of one kind; with and without pbf_pre.  No tolerance appears anywhere.
"""
import numpy as np
import pytest

import family_ranges_kit as K
import mixed_kinds_kit as M
from mixed_kinds_kit import COMMANDS, GLYF, GROUP, compare_ranges, random_mixed_family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kit(vg):
    ctx = vg.SdfContext(0)
    try:
        yield M.MixedKit(vg, ctx)
    finally:
        ctx.close()


def span(fam, i, count, pre=0, k=0):
    """the task of family k over exactly its entries [i, i + count)"""
    return (k, int(fam.cp[i]), int(fam.cp[i + count - 1]), pre)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_one_task_of_n_glyphs_with_font_of_alternating(kit, n):
    fam = random_mixed_family(kit, n, 300)
    assert (np.diff(fam.font_of) != 0).all()
    rects = compare_ranges(kit.ctx, [fam], [span(fam, 7, n, pre=19)])
    assert len(rects) == n and int(rects["has_raster"].sum()) == n
    assert fam.handle.count(int(fam.cp[7]), int(fam.cp[7 + n - 1])) == n and fam.handle.device_bytes >= 27 * 300 + 8 * 301


def test_the_table_a_mixed_family_keeps(kit):
    """cmd_pre over the slots of every entry, leaf_pre over the leaves of the glyf entries alone"""
    fam = random_mixed_family(kit, 2, 200, big_at=[10, 11], empty_at=[20, 21])
    t = kit.ctx.family_read(fam.handle)
    kind = np.array([k for k, _ in fam.font_list])[fam.font_of]
    glyf_font = kit.ctx.font_read(kit.kits[GLYF].kinds[0])
    leaves = np.diff(glyf_font["leaf_off"].astype(np.int64))
    assert np.array_equal(np.diff(t["cmd_pre"].astype(np.int64)), [kit.slots(int(k), int(g)) for k, g in zip(kind, fam.gid)])
    assert np.array_equal(np.diff(t["leaf_pre"].astype(np.int64)), np.where(kind == GLYF, leaves[np.where(kind == GLYF, fam.gid, 0)], 0))
    assert np.array_equal(t["code_point"], fam.cp) and np.array_equal(t["font_of"], fam.font_of) and np.array_equal(t["glyph_id"], fam.gid)
    assert t["pbf_fix"].tobytes() == K.fix_of(fam.cp, fam.advance).tobytes()


def test_tasks_straddle_workgroups(kit):
    """tasks that end on, one before and one behind every multiple of 256 glyphs; one task over three workgroups"""
    fam = random_mixed_family(kit, 11, 900)
    sizes = [255, 1, 1, 255, 1, 256, 257, 254, 1, 2, 253]
    tasks, at = [], 0
    for j, s in enumerate(sizes):
        tasks.append(span(fam, at % 600, s, pre=10 + j))
        at += 97
    rects = compare_ranges(kit.ctx, [fam], tasks)
    assert len(rects) == sum(sizes)
    for cut in (255, 257):
        compare_ranges(kit.ctx, [fam], [span(fam, 0, cut, pre=5), span(fam, 300, 300, pre=6)], layouts=(cut == 255,))
    assert len(compare_ranges(kit.ctx, [fam], [span(fam, 50, 700, pre=33)], layouts=(True,))) == 700


def test_300_one_glyph_tasks(kit):
    fam = random_mixed_family(kit, 5, 400)
    order = np.random.default_rng(1).permutation(300)
    rects = compare_ranges(kit.ctx, [fam], [span(fam, int(i), 1, pre=int(i) % 40) for i in order])
    assert len(rects) == 300


def test_two_mixed_families_in_one_submission(kit):
    """their font lists differ in order and in fonts, and share one font"""
    a = random_mixed_family(kit, 20, 300, font_list=[(GLYF, 0), (COMMANDS, 1), (GLYF, 2)])
    b = random_mixed_family(kit, 21, 300, font_list=[(COMMANDS, 1), (COMMANDS, 2), (GLYF, 1)], first_cp=40)
    tasks = [span(a, 0, 250, pre=4), span(b, 10, 250, pre=5, k=1), span(a, 250, 50, pre=6), span(b, 0, 10, pre=7, k=1)]
    compare_ranges(kit.ctx, [a, b], tasks)
    compare_ranges(kit.ctx, [b, a], [(1 - k, f, l, p) for k, f, l, p in tasks], layouts=(True,))
    # one family listed twice is two families of the block
    compare_ranges(kit.ctx, [a, a], [span(a, 0, 20, pre=4), span(a, 5, 20, pre=5, k=1)], layouts=(True,))


def test_repeated_overlapping_and_descending_tasks(kit):
    fam = random_mixed_family(kit, 10, 500)
    t = span(fam, 20, 90, pre=17)
    tasks = [t, t, t, span(fam, 60, 100, pre=1), span(fam, 100, 30, pre=2), span(fam, 0, 500, pre=3)]
    compare_ranges(kit.ctx, [fam], tasks)
    compare_ranges(kit.ctx, [fam], [span(fam, 400 - 40 * j, 40, pre=j) for j in range(10)], layouts=(True,))


@pytest.mark.parametrize("kind", [GLYF, COMMANDS])
def test_a_mixed_family_whose_fonts_are_all_of_one_kind(kit, kind):
    """it is of the mixed kind all the same: it renders what the family of its kind renders, and stands beside mixed families only"""
    fam = random_mixed_family(kit, 30 + kind, 400, font_list=[(kind, 0), (kind, 2)], big_at=[50], empty_at=[0, 399])
    tasks = [span(fam, 0, 300, pre=8), span(fam, 390, 10, pre=9)]
    rects = compare_ranges(kit.ctx, [fam], tasks)
    # the single-kind family of the same entries, through the existing forms
    single = kit.ctx.family_create(fam.fonts, fam.cp, fam.font_of, fam.gid, fam.advance, fam.scale, fam.shift)
    fam_of, first, last, room = [np.array([t[i] for t in tasks], np.int64) for i in range(4)]
    kit.ctx.outlines_submit_ranges([single], fam_of, first, last, capacity=M.CAPACITY)
    got = kit.ctx.outlines_wait()
    assert np.array_equal(got[0], rects)
    both = random_mixed_family(kit, 33, 100)
    compare_ranges(kit.ctx, [fam, both], [span(fam, 10, 100, pre=1), span(both, 0, 100, pre=2, k=1)], layouts=(True,))
    single.free()


def test_tasks_that_map_nothing(kit):
    fam = random_mixed_family(kit, 8, 300, first_cp=1000, gaps=(2, 3))
    hole = int(next(c for c in range(1001, 3000) if c not in set(fam.cp.tolist())))
    nothing = [(0, 0, 999, 9), (0, hole, hole, 11), (0, int(fam.cp[-1]) + 1, 0xFFFF, 13)]
    full = [span(fam, 3, 40, pre=21), span(fam, 100, 200, pre=22)]
    for tasks in ([nothing[0], nothing[1], full[0], nothing[2], nothing[0], full[1], nothing[1]],):
        assert len(compare_ranges(kit.ctx, [fam], tasks)) == 240
    for tasks in ([nothing[1]], nothing, []):
        assert len(compare_ranges(kit.ctx, [fam], tasks)) == 0
    assert len(compare_ranges(kit.ctx, [fam], full[:1], layouts=(True,))) == 40


def test_glyphs_without_outline_and_very_large_glyphs_of_both_kinds(kit):
    """pbf_pre lands on a glyph without a raster of either kind; the 600-leaf glyph between command entries and the 5000-command
    glyph between glyf entries, inside a workgroup, as its last glyph and as the first of the next"""
    big_at = [31, 60, 100 + GROUP - 1, 100 + GROUP]
    empty_at = [10, 49, 50, 99, 100, 399]
    fam = random_mixed_family(kit, 12, 400, big_at=big_at, empty_at=empty_at)
    kind = np.array([k for k, _ in fam.font_list])[fam.font_of]
    assert {int(kind[i]) for i in big_at} == {GLYF, COMMANDS} and {int(kind[i]) for i in empty_at} == {GLYF, COMMANDS}
    tasks = [span(fam, 10, 40, pre=23), span(fam, 50, 50, pre=24), span(fam, 100, 300, pre=25), span(fam, 399, 1, pre=26), span(fam, 49, 2, pre=0)]
    rects = compare_ranges(kit.ctx, [fam], tasks)
    firsts = np.cumsum([0] + [fam.handle.count(t[1], t[2]) for t in tasks])[:-1]
    assert (rects["has_raster"][firsts] == 0).all() and rects["has_raster"][-1] == 0
    compare_ranges(kit.ctx, [fam], [span(fam, 31, 1, pre=12), span(fam, 60, 1, pre=1)], layouts=(True,))


@pytest.mark.parametrize("n_fonts", [129, 200])
def test_families_around_the_font_cache(kit, n_fonts):
    """a family over n_fonts fonts with the kinds interleaved, and a second family behind it whose fonts begin at n_fonts in the
    block's list — either side of the 128 references a workgroup keeps in LDS, both kinds on both sides"""
    font_list = [(i % 2, (i // 2) % 3) for i in range(n_fonts)]
    a = random_mixed_family(kit, n_fonts, 600, font_list=font_list, font_of=(np.arange(600) * 7 + n_fonts) % n_fonts)
    b = random_mixed_family(kit, n_fonts + 1, 100, font_list=[(COMMANDS, 2), (GLYF, 0)])
    assert set(a.font_of.tolist()) == set(range(n_fonts))
    tasks = [span(a, 0, 600, pre=9), span(b, 0, 100, pre=8, k=1), span(a, 300, 10, pre=7), span(b, 50, 50, pre=6, k=1)]
    compare_ranges(kit.ctx, [a, b], tasks, layouts=(n_fonts == 129,))
    compare_ranges(kit.ctx, [b, a], [(1 - k, f, l, p) for k, f, l, p in tasks], layouts=(n_fonts != 129,))


def test_a_mixed_family_beside_a_family_of_one_kind_is_refused_and_the_context_goes_on(vg, kit):
    mixed = random_mixed_family(kit, 40, 100)
    one_kind_mixed = random_mixed_family(kit, 41, 100, font_list=[(GLYF, 0)])
    singles = []
    for kind in (GLYF, COMMANDS):
        f = random_mixed_family(kit, 42 + kind, 100, font_list=[(kind, 0)])
        singles.append(kit.ctx.family_create(f.fonts, f.cp, f.font_of, f.gid, f.advance, f.scale, f.shift))
    for fams in ([mixed.handle, singles[0]], [singles[1], mixed.handle], [singles[0], one_kind_mixed.handle], [mixed.handle, singles[1], mixed.handle],
                 [singles[0], singles[1]]):
        for fam_of in ([0], list(range(len(fams)))):       # named by a task or not
            with pytest.raises(vg.VgsdfError) as e:
                kit.ctx.outlines_submit_ranges(fams, fam_of, [0] * len(fam_of), [0xFFFF] * len(fam_of), capacity=M.CAPACITY)
            assert e.value.code == M.E_ARG
        compare_ranges(kit.ctx, [mixed], [span(mixed, 0, 100, pre=3)], layouts=(True,))       # the context is sound
    compare_ranges(kit.ctx, [mixed, one_kind_mixed], [span(mixed, 0, 50, pre=3), span(one_kind_mixed, 20, 50, pre=1, k=1)])
    for s in singles:
        s.free()
