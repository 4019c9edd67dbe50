"""The upload kernel of resident submissions (resident_expand, csrc/input_form_kernels.hip) at its edges: 256 glyphs per workgroup,
the bisection over offsets that glyphs without leaves share, glyphs of more leaves than a workgroup has lanes, the 128 font
references a workgroup keeps in LDS and the load from the block behind them, both block layouts (with and without the in-place
PBF arrays) and their 16-byte tails.

The yardstick is the glyf form of the same glyph list (vgsdf_outlines_submit_glyf, pinned to the host's reader and to the
strict decoder by the glyf tests): rects, sizes, every segment bit for bit, every bitmap — tests/test_gpu_resident_fonts.py's
comparison, imported.
"""
import numpy as np
import pytest

import glyf_edge_entries as E
from test_gpu_resident_fonts import _assert_same, _font_set, _glyf_subset, _run_glyf, _run_resident, _upload

pytestmark = pytest.mark.gpu

GROUP = 256          # glyphs per workgroup of the upload kernel (kExpandThreads)
CAPACITY = 8 << 20


def _pbf(n):
    """in-place PBF arrays for n glyphs: room for a block header in front of every 100th, two-byte fields"""
    pre = np.zeros(n, np.uint32)
    pre[::100] = 23
    fix = np.full(n, 2 | (3 << 4), np.uint8)
    fix[1::3] = 3 | (2 << 4)
    return dict(pbf_pre=pre, pbf_fix=fix)


def _both_layouts(ctx, fonts, r, sel, form):
    for pbf in ({}, _pbf(len(sel))):
        want = _run_glyf(ctx, form, CAPACITY, **pbf)
        got = _run_resident(ctx, fonts, r, sel, CAPACITY, **pbf)
        _assert_same(got, want)
    return want


def test_the_restated_constants_are_the_kernels(vg):
    import ctypes as C
    cache = C.c_uint32()
    vg.load_library().vgsdf_glyf_limits(None, None, C.byref(cache))
    assert cache.value == E.EXPAND_FONT_CACHE == 128


@pytest.fixture(scope="module")
def noto(vg):
    _, _, g, r, descs = _font_set(vg, "noto_regular")
    n_parts = np.diff(np.searchsorted(g["parts"]["cmd_at"], g["cmd_off"].astype(np.int64)))
    return g, r, descs, n_parts


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 512, 513, 2500])
def test_glyph_counts_around_the_workgroup_size(vg, noto, n):
    g, r, descs, n_parts = noto
    rng = np.random.default_rng(n)
    sel = rng.integers(0, len(r["ids"]), n)            # any order, repeats
    sel[0] = int(np.flatnonzero(n_parts >= 2)[n % 50])   # (a single glyph: one with several leaves)
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        want = _both_layouts(ctx, fonts, r, sel, _glyf_subset(g, sel))
        assert int(want[0][0]["has_raster"].sum()) >= min(n, 1)
    finally:
        ctx.close()


def _with_empties(rng, n, n_parts, empty_at):
    full = np.flatnonzero(n_parts >= 1)
    empties = np.flatnonzero(n_parts == 0)
    sel = rng.choice(full, n)
    at = np.array(sorted(empty_at), dtype=np.int64)
    sel[at] = rng.choice(empties, len(at))
    return sel


EMPTY_POSITIONS = {
    "first_of_a_workgroup": (600, [0, GROUP, 2 * GROUP]),
    "last_of_a_workgroup": (600, [GROUP - 1, 2 * GROUP - 1, 599]),
    "a_run_across_the_boundary": (600, list(range(GROUP - 6, GROUP + 7))),
    "first_and_last_and_the_run": (700, [0] + list(range(GROUP - 2, GROUP + 2)) + list(range(2 * GROUP - 9, 2 * GROUP)) + [2 * GROUP] + [699]),
    "a_whole_workgroup": (3 * GROUP + 10, list(range(GROUP, 2 * GROUP))),
    "two_whole_workgroups_and_the_tail": (3 * GROUP + 10, list(range(GROUP, 3 * GROUP + 10))),
    "the_whole_submission": (300, list(range(300))),
    "a_single_glyph": (1, [0]),
}


@pytest.mark.parametrize("where", list(EMPTY_POSITIONS))
def test_glyphs_without_leaves(vg, noto, where):
    g, r, descs, n_parts = noto
    n, empty_at = EMPTY_POSITIONS[where]
    assert int((n_parts == 0).sum()) >= 5
    sel = _with_empties(np.random.default_rng(len(where)), n, n_parts, empty_at)
    assert (n_parts[sel[empty_at]] == 0).all() and int((n_parts[sel] == 0).sum()) == len(empty_at)
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        want = _both_layouts(ctx, fonts, r, sel, _glyf_subset(g, sel))
        rects = want[0][0]
        assert (rects["n_segments"][empty_at] == 0).all() and int((rects["n_segments"] > 0).sum()) >= (n - len(empty_at)) * 9 // 10
    finally:
        ctx.close()


# ---- synthetic composite fonts: many small leaves per glyph id, several fonts of one structure ----

LEAF_CASES = ["D_cmd_cap_exact", "D_every_coordinate_byte_there", "C_open_end_smallest_cmd_cap", "D_run_ends_on_the_last_point",
              "C_one_off_curve_point_then_a_contour", "A_fake_runs_of_256_cross_the_point_count", "A_count_bit3_in_the_middle"]
LEAVES_PER_GLYPH = [0, 300, 600, 2, 3, 4, 5, 1, 0, 1, 2, 5, 257, 1, 3, 0, 4, 2, 1, 513]
N_KINDS = 3   # fonts that differ in their leaves' transforms only: a mixed-up reference stays inside every buffer and moves the outlines


def _synthetic(vg):
    """-> descriptions of N_KINDS fonts (leaf_off, leaves, store) and the table of their glyphs in the glyf form (as
    record_glyf_parts lists a font's glyphs: parts, cmd_off, bytes, scale, shift_x); glyph gid of font k is row k * n_ids + gid"""
    from versatiles_glyphs_rs_amd.device import GLYF_PART_DTYPE
    cases = [E.BY_NAME[n] for n in LEAF_CASES]
    store, at = bytearray(), []
    for c in cases:
        at.append(len(store))
        store += c.part + b"\0" * (-len(c.part) % 4)
    store = np.frombuffer(bytes(store), np.uint8)
    descs, parts, cmd_off, slots = [], [], [0], 0
    for k in range(N_KINDS):
        leaves, leaf_off = [], [0]
        for gid, n_leaves in enumerate(LEAVES_PER_GLYPH):
            in_glyph = 0
            for j in range(n_leaves):
                ci = (gid + 3 * j) % len(cases)
                lf = np.zeros((), dtype=GLYF_PART_DTYPE)
                lf["byte_off"], lf["byte_len"] = at[ci], len(cases[ci].part)
                lf["cmd_at"], lf["cmd_cap"], lf["n_contours"] = in_glyph, cases[ci].cmd_cap + j % 2, cases[ci].n_contours
                lf["a"], lf["d"] = 1.0, (1.0, -1.0, 0.5)[k]
                lf["e"], lf["f"] = 35.0 * (j % 24) + 11.0 * k, 30.0 * ((j // 24) % 20) + 400.0 * (k == 1)
                leaves.append(lf)
                p = lf.copy()
                p["byte_off"] = int(lf["byte_off"]) + k * len(store)
                p["cmd_at"] = slots + in_glyph
                parts.append(p)
                in_glyph += int(lf["cmd_cap"])
            slots += in_glyph
            cmd_off.append(slots)
            leaf_off.append(len(leaves))
        descs.append((np.array(leaf_off, np.uint32), np.array(leaves, dtype=GLYF_PART_DTYPE), store))
    n_rows = N_KINDS * len(LEAVES_PER_GLYPH)
    table = {"parts": np.array(parts, dtype=GLYF_PART_DTYPE), "cmd_off": np.array(cmd_off, np.uint32), "bytes": np.tile(store, N_KINDS),
             "scale": np.full(n_rows, 24.0 / 1000.0) * np.array([1.0, 0.5, 0.75])[np.arange(n_rows) % 3],
             "shift_x": ((np.arange(n_rows) * 37) % 100) / 100.0 - 0.5}
    return descs, table


def _submit_synthetic(ctx, kinds, table, font_list, font_of, gid):
    """font_list: kind of every entry of the submission's font list; glyph i is glyph id gid[i] of entry font_of[i]"""
    font_of, gid = np.asarray(font_of), np.asarray(gid)
    rows = np.asarray(font_list)[font_of] * len(LEAVES_PER_GLYPH) + gid
    r = {"font_of": font_of.astype(np.uint16), "glyph_id": gid.astype(np.uint16), "scale": table["scale"][rows], "shift_x": table["shift_x"][rows]}
    want = _both_layouts(ctx, [kinds[k] for k in font_list], r, np.arange(len(gid)), _glyf_subset(table, rows))
    return want[0][0]


def test_glyphs_of_more_leaves_than_a_workgroup_has_lanes(vg):
    descs, table = _synthetic(vg)
    L = np.array(LEAVES_PER_GLYPH)
    big = [int(i) for i in np.flatnonzero(L > GROUP)]
    assert sorted(L[big]) == [257, 300, 513, 600]       # the dealing loop's second and third round
    ctx = vg.SdfContext(0)
    try:
        kinds = [ctx.font_create(*d) for d in descs]
        for gids in ([1], [12], [2, 19], big, [3, 1, 0, 2, 7], list(range(len(L))) * 3):
            rects = _submit_synthetic(ctx, kinds, table, [0], np.zeros(len(gids), int), gids)
            assert ((rects["n_segments"] > 0) == (L[gids] > 0)).all()
        # glyphs of 2 to 5 leaves on either side of a workgroup boundary, singles and glyphs without leaves around them
        small = [int(i) for i in np.flatnonzero((L >= 2) & (L <= 5))]
        assert sorted(set(L[small])) == [2, 3, 4, 5]
        for shift in range(len(small)):
            gids = np.array([7, 9, 13, 8, 18] * 120)[:2 * GROUP + 40]
            for b in (GROUP, 2 * GROUP):
                for o in range(-3, 3):
                    gids[b + o] = small[(o + 3 + shift) % len(small)]
            rects = _submit_synthetic(ctx, kinds, table, [1], np.zeros(len(gids), int), gids)
            assert ((rects["n_segments"] > 0) == (L[gids] > 0)).all()
        # a many-leaved glyph as the last of a workgroup and as the first of the next
        gids = np.array([7] * (2 * GROUP + 5))
        gids[GROUP - 1], gids[GROUP], gids[2 * GROUP - 1] = 2, 1, 19
        _submit_synthetic(ctx, kinds, table, [2], np.zeros(len(gids), int), gids)
    finally:
        ctx.close()


@pytest.mark.parametrize("n_fonts", [1, 127, 128, 129, 200])
def test_font_lists_around_the_cache_size(vg, n_fonts):
    """the same three handles listed again and again: entry i is kind i % 3, so the entries around the cache's end (127 | 128)
    and the list's ends are fonts whose outlines differ"""
    descs, table = _synthetic(vg)
    L = np.array(LEAVES_PER_GLYPH)
    font_list = [i % N_KINDS for i in range(n_fonts)]
    wanted = [i for i in (0, 1, 126, 127, 128, 129, 199) if i < n_fonts]
    assert len({font_list[i] for i in wanted}) >= min(n_fonts, 2)
    rng = np.random.default_rng(n_fonts)
    ctx = vg.SdfContext(0)
    try:
        kinds = [ctx.font_create(*d) for d in descs]
        # cached and uncached indices side by side in every workgroup (the ends of the list, both sides of the cache's end)
        n = 2 * GROUP + 77
        font_of = np.array(wanted)[np.arange(n) % len(wanted)]
        gids = rng.choice(np.flatnonzero(L <= 5), n)
        rects = _submit_synthetic(ctx, kinds, table, font_list, font_of, gids)
        assert ((rects["n_segments"] > 0) == (L[gids] > 0)).all()
        # every index of the list once, and the many-leaved glyphs from the list's last font
        font_of = np.concatenate([np.arange(n_fonts), [n_fonts - 1] * 3])
        gids = np.concatenate([rng.choice(np.flatnonzero((L >= 1) & (L <= 5)), n_fonts), [1, 12, 2]])
        _submit_synthetic(ctx, kinds, table, font_list, font_of, gids)
        if n_fonts == 200:
            font_of = np.array([0, 127, 128, 199] * 80)
            assert [font_list[i] for i in (0, 127, 128, 199)] == [0, 1, 2, 1]
            _submit_synthetic(ctx, kinds, table, font_list, font_of, rng.choice(np.flatnonzero((L >= 1) & (L <= 5)), len(font_of)))
    finally:
        ctx.close()
