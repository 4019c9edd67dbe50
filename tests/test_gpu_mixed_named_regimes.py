"""vgsdf_outlines_submit_resident_mixed — glyphs named one by one against fonts of BOTH kinds in one list — and its upload kernel
(resident_mixed, csrc/input_form_kernels.hip) at their edges: 256 glyphs per workgroup with the kinds alternating and in runs that
change on the boundary, workgroups without a part and without a gathered record, the gather's range spanning slots that are the
decoder's (a 600-leaf glyf glyph between command glyphs, the 5000-command glyph between glyf glyphs, glyf slots beginning at every
position of a gather round), glyphs without outline at the ends, the 128 font references of the one LDS cache with both kinds on
either side of it, the context-pass route, lists of one kind, and the refusals.

The fonts are synthetic (tests/mixed_kinds_kit.py).  The yardstick of a sequence is its glyf and its command subsequence, each
submitted by the existing vgsdf_outlines_submit_resident and interleaved back: rects, every segment bit for bit, every bitmap;
the positions of the in-place PBF arena come from a restatement of include/vgsdf.h that is first held against each single-kind
submission.  No tolerance appears anywhere.
"""
import numpy as np
import pytest

import mixed_kinds_kit as M
from mixed_kinds_kit import COMMANDS, GLYF, GROUP, ROUND, compare

pytestmark = pytest.mark.gpu

BOTH = [(GLYF, 0), (COMMANDS, 0)]


@pytest.fixture(scope="module")
def kit(vg):
    ctx = vg.SdfContext(0)
    try:
        yield M.MixedKit(vg, ctx)
    finally:
        ctx.close()


def test_the_restated_constants_are_the_kernels(vg):
    import ctypes as C
    cache = C.c_uint32()
    vg.load_library().vgsdf_glyf_limits(None, None, C.byref(cache))
    assert cache.value == M.FONT_CACHE


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("first", [GLYF, COMMANDS])
def test_kinds_alternating_glyph_by_glyph(kit, n, first):
    kinds = (np.arange(n) + first) % 2
    font_list, font_of, gid = M.glyphs(kit, np.random.default_rng(n), kinds)
    rects = compare(kit, font_list, font_of, gid)
    assert int(rects["has_raster"].sum()) == n


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_kinds_in_runs_that_change_on_the_workgroup_boundary(kit, n):
    """workgroup 0 has no gathered record, workgroup 1 no part (and the other way round); the tail is of the first kind again"""
    for first in (GLYF, COMMANDS):
        kinds = (np.arange(n) // GROUP + first) % 2
        font_list, font_of, gid = M.glyphs(kit, np.random.default_rng(n + first), kinds)
        rects = compare(kit, font_list, font_of, gid, layouts=(first == GLYF,))
        assert int(rects["has_raster"].sum()) == n


def test_a_workgroup_without_a_part_and_one_without_a_record_between_mixed_ones(kit):
    kinds = np.concatenate([np.arange(GROUP) % 2, np.full(GROUP, COMMANDS), np.arange(GROUP) % 2, np.full(GROUP, GLYF), np.arange(40) % 2])
    font_list, font_of, gid = M.glyphs(kit, np.random.default_rng(3), kinds)
    compare(kit, font_list, font_of, gid)


def test_the_600_leaf_glyph_between_command_glyphs(kit):
    """the gather's range [cmd_off of the first command glyph, end of the last) spans the slots of the glyf glyph: they are passed
    over, and what lies behind them is gathered to the right place"""
    big, c = kit.big[GLYF], kit.small[COMMANDS]
    assert kit.slots(GLYF, big) > ROUND
    for kinds, gid in (([COMMANDS, GLYF, COMMANDS], [c[0], big, c[1]]),
                       ([COMMANDS, COMMANDS, GLYF, GLYF, COMMANDS], [c[2], c[3], big, big, c[4]]),
                       # the large glyph as the last glyph of a workgroup and as the first of the next
                       ([COMMANDS] * (GROUP - 1) + [GLYF, GLYF] + [COMMANDS] * 9, [c[1]] * (GROUP - 1) + [big, big] + [c[2]] * 9)):
        compare(kit, BOTH, kinds, gid)


def test_the_5000_command_glyph_between_glyf_glyphs(kit):
    big, g = kit.big[COMMANDS], kit.small[GLYF]
    for kinds, gid in (([GLYF, COMMANDS, GLYF], [g[0], big, g[1]]),
                       ([GLYF, GLYF, COMMANDS, COMMANDS, GLYF], [g[2], g[3], big, big, g[4]]),
                       ([GLYF] * (GROUP - 1) + [COMMANDS, COMMANDS] + [GLYF] * 9, [g[1]] * (GROUP - 1) + [big, big] + [g[2]] * 9)):
        compare(kit, BOTH, kinds, gid)


def test_glyf_slots_begin_at_every_position_of_a_gather_round(kit):
    """a workgroup gathers kGatherUnroll * 256 = 1024 commands per round, from its first glyph's offset on: pairs of a command
    glyph and a glyf glyph, the command glyphs' lengths chosen so that over the submission the glyf glyphs' first slots fall on
    every one of the 1024 positions (asserted)"""
    lengths = kit.command_lengths
    usable = [int(i) for i in np.flatnonzero((lengths >= 1) & (lengths <= 100))]
    g = int(kit.small[GLYF][0])
    s = kit.slots(GLYF, g)
    seen, gid, kinds = set(), [], []
    while len(seen) < ROUND:
        assert len(gid) < 40 * GROUP
        at = 0                                  # (a workgroup: 128 pairs)
        for _ in range(GROUP // 2):
            pick = next((i for i in usable if (at + int(lengths[i])) % ROUND not in seen), usable[len(gid) % len(usable)])
            at += int(lengths[pick])
            seen.add(at % ROUND)
            at += s
            gid += [pick, g]
            kinds += [COMMANDS, GLYF]
    assert seen == set(range(ROUND))
    compare(kit, BOTH, kinds, gid, layouts=(False,))


def test_glyphs_without_outline_first_and_last(kit):
    e, sm = kit.empty, kit.small
    for first, last in ((GLYF, COMMANDS), (COMMANDS, GLYF), (GLYF, GLYF), (COMMANDS, COMMANDS)):
        kinds = [first] + [GLYF, COMMANDS] * 150 + [last]
        gid = [int(e[first][0])] + [int(sm[GLYF][1]), int(sm[COMMANDS][1])] * 150 + [int(e[last][-1])]
        rects = compare(kit, BOTH, kinds, gid)
        assert rects["has_raster"][0] == 0 and rects["has_raster"][-1] == 0 and int(rects["has_raster"].sum()) == 300
    # nothing but glyphs without outline, of both kinds
    rects = compare(kit, BOTH, [GLYF, COMMANDS, COMMANDS, GLYF], [int(e[GLYF][0]), int(e[COMMANDS][0]), int(e[COMMANDS][1]), int(e[GLYF][1])])
    assert int(rects["has_raster"].sum()) == 0


@pytest.mark.parametrize("n_fonts", [128, 129, 133])
def test_font_lists_around_the_cache_size_with_the_kinds_interleaved(kit, n_fonts):
    """entry i of the list is of kind i % 2 and of the kit's font (i // 2) % 3: fonts of both kinds sit on either side of the 128
    references a workgroup keeps in LDS, and neighbours of one kind differ in their outlines"""
    font_list = [(i % 2, (i // 2) % 3) for i in range(n_fonts)]
    wanted = [i for i in (0, 1, 2, 3, 126, 127, 128, 129, 130, 131, 132) if i < n_fonts]
    rng = np.random.default_rng(n_fonts)
    n = 2 * GROUP + 77
    font_of = np.array(wanted)[np.arange(n) % len(wanted)]      # cached and uncached indices side by side in every workgroup
    kinds = font_of % 2
    gid = np.where(kinds == GLYF, rng.choice(kit.small[GLYF], n), rng.choice(kit.small[COMMANDS], n))
    compare(kit, font_list, font_of, gid)
    if n_fonts > M.FONT_CACHE + 1:
        assert {k for k, _ in font_list[M.FONT_CACHE:]} == {GLYF, COMMANDS}
    # every index of the list once, and the large glyphs from the list's last fonts of either kind
    last = {font_list[i][0]: i for i in range(n_fonts)}
    font_of = np.concatenate([np.arange(n_fonts), [last[GLYF], last[COMMANDS]]])
    kinds = font_of % 2
    gid = np.where(kinds == GLYF, rng.choice(kit.small[GLYF], len(kinds)), rng.choice(kit.small[COMMANDS], len(kinds)))
    gid[-2:] = [kit.big[GLYF], kit.big[COMMANDS]]
    compare(kit, font_list, font_of, gid, layouts=(True,))


def test_odd_scales_take_the_context_pass(kit):
    """a negative scale on a glyph with an outline and an infinite one on a glyph without, of either kind in turn: neither the
    decoder's nor the gathered context bytes have the bit only the context pass forms, so it runs over the whole batch"""
    n = GROUP + 40
    for neg_kind in (GLYF, COMMANDS):
        kinds = np.arange(n) % 2
        font_list, font_of, gid = M.glyphs(kit, np.random.default_rng(neg_kind), kinds)
        scale, shift = M.scales(n)
        scale = scale.copy()
        neg, inf = 20 + neg_kind, 101 - neg_kind       # (the infinite one on the other kind)
        assert kinds[neg] == neg_kind and kinds[inf] == 1 - neg_kind
        gid[inf] = kit.empty[1 - neg_kind][0]
        scale[neg] *= -1.0
        scale[inf] = np.inf
        compare(kit, font_list, font_of, gid, scale=scale, shift=shift)


@pytest.mark.parametrize("kind", [GLYF, COMMANDS])
def test_a_list_of_one_kind_equals_the_existing_call(kit, kind):
    n = GROUP + 31
    rng = np.random.default_rng(kind)
    font_list = [(kind, 0), (kind, 2), (kind, 1)]
    font_of = rng.integers(0, 3, n)
    gid = rng.choice(kit.small[kind], n)
    gid[[5, n - 1]] = kit.big[kind], kit.empty[kind][0]
    scale, shift = M.scales(n)
    fonts = kit.handles(font_list)
    for pbf in ({}, M.pbf_arrays(n)):
        want = M.run_resident(kit.ctx, fonts, font_of, gid, scale, shift, **pbf)
        got = M.run_resident(kit.ctx, fonts, font_of, gid, scale, shift, mixed=True, **pbf)
        M._assert_same(got, want)
    compare(kit, font_list, font_of, gid, layouts=(True,))      # (and the yardstick agrees with both)


def test_an_empty_submission(kit):
    got = M.run_resident(kit.ctx, kit.handles(BOTH), [], [], np.zeros(0), np.zeros(0), mixed=True)
    assert len(got[0][0]) == 0 and got[0][2] == 0


def test_bad_submissions_are_refused_and_the_context_goes_on(vg, kit):
    import ctypes as C
    from versatiles_glyphs_rs_amd.device import _COutlinesResident
    ctx = kit.ctx
    fonts = kit.handles(BOTH)
    scale, shift = M.scales(4)
    good = ([GLYF, COMMANDS, COMMANDS, GLYF], [int(kit.small[GLYF][0]), int(kit.small[COMMANDS][0]), kit.big[COMMANDS], int(kit.small[GLYF][2])])

    def refused(font_of, gid):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.outlines_submit_resident_mixed(fonts, font_of, gid, scale, shift, capacity=1 << 20)
        assert e.value.code == M.E_ARG
        compare(kit, BOTH, *good, layouts=(True,))

    refused([0, 1, 0, 1], [1, 2, kit.n_ids[GLYF], 3])            # a glyph id past its (glyf) face
    refused([0, 1, 0, 1], [1, kit.n_ids[COMMANDS], 2, 3])        # ... past its (command) face
    # (an id inside the larger face and past the smaller one is refused for the smaller alone)
    lo, hi = sorted((GLYF, COMMANDS), key=lambda k: kit.n_ids[k])
    if kit.n_ids[lo] < kit.n_ids[hi]:
        refused([lo, lo, lo, lo], [1, 2, kit.n_ids[lo], 3])
    refused([0, 2, 0, 1], [1, 2, 3, 4])                          # font_of past n_fonts
    # NULL arrays, a NULL font, a NULL description
    L = vg.load_library()
    handles = (C.c_void_p * 2)(*[f._h for f in fonts])
    fo, gi = np.array([0, 1, 0, 1], np.uint16), np.array([1, 2, 3, 4], np.uint16)
    p = lambda a: a.ctypes.data  # noqa: E731
    out = L.vgsdf_host_alloc(1 << 16)
    try:
        for null in ("fonts", "font_of", "glyph_id", "scale", "shift_x"):
            d = _COutlinesResident(4, 2, C.cast(handles, C.c_void_p), p(fo), p(gi), p(scale), p(shift))
            setattr(d, null, None)
            assert L.vgsdf_outlines_submit_resident_mixed(ctx._h, C.byref(d), out, 1 << 16) == M.E_ARG
        holed = (C.c_void_p * 2)(fonts[0]._h, None)
        d = _COutlinesResident(4, 2, C.cast(holed, C.c_void_p), p(fo), p(gi), p(scale), p(shift))
        assert L.vgsdf_outlines_submit_resident_mixed(ctx._h, C.byref(d), out, 1 << 16) == M.E_ARG
        assert L.vgsdf_outlines_submit_resident_mixed(ctx._h, None, out, 1 << 16) == M.E_ARG
        pre = np.zeros(4, np.uint32)                             # pbf_pre without pbf_fix
        d = _COutlinesResident(4, 2, C.cast(handles, C.c_void_p), p(fo), p(gi), p(scale), p(shift), p(pre), None)
        assert L.vgsdf_outlines_submit_resident_mixed(ctx._h, C.byref(d), out, 1 << 16) == M.E_ARG
    finally:
        L.vgsdf_host_free(out)
    compare(kit, BOTH, *good)


def test_the_existing_call_still_refuses_both_kinds(vg, kit):
    ctx = kit.ctx
    scale, shift = M.scales(4)
    g, c = int(kit.small[GLYF][0]), int(kit.small[COMMANDS][0])
    for fonts, font_of, gid in ((BOTH, [0, 1, 0, 1], [g, c, g, c]), (BOTH[::-1], [0, 0, 0, 0], [c, c, c, c]), (BOTH, [0, 0, 0, 0], [g, g, g, g])):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.outlines_submit_resident(kit.handles(fonts), font_of, gid, scale, shift, capacity=1 << 20)
        assert e.value.code == M.E_ARG
    compare(kit, BOTH, [GLYF, COMMANDS], [g, c], layouts=(False,))
