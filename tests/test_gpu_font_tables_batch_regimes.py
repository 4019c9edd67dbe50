"""Glyf fonts of SEVERAL faces built by one call (vgsdf_fonts_create_tables; the multi-face kernels of
csrc/glyf_table_kernels.hip) at the edges of what is new in it: which workgroup belongs to which face (faces that end on a
workgroup's edge, faces without glyph ids first, last, between two others and side by side), unlike neighbours in one launch, a
composite that names a glyph id only its neighbour has, refusals and bad descriptions between good faces, the limit taken face by
face, the whole call's arguments, submissions over the fonts of one batch, and the passes' timers.

Every face a batch builds must equal BOTH yardsticks, read back with vgsdf_font_read and compared array by array, byte for byte,
and in device_bytes: vgsdf_font_create of the arrays the Python restatement gives for its tables (tests/composite_edge_trees.py,
pinned to the host reader by tests/test_font_tables_desc_host.py) and vgsdf_font_create_tables of the same face alone.  No
tolerance appears anywhere."""
import numpy as np
import pytest

import composite_edge_trees as T

pytestmark = pytest.mark.gpu

OK, E_ARG, E_GLYF = 0, -1, -4
EMPTY = T.Tables(b"", b"", 0, 0, 1)          # a face without glyph ids: no workgroup is its own


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


def store_bytes(r):
    """GlyfStoreLayout's total of restated arrays: the formula of test_a_limit_on_the_store_is_checked_before_it_is_allocated"""
    return (48 * len(r["leaves"]) + len(r["bytes"]) + 15) // 16 * 16 + 4 * len(r["leaf_off"])


def assert_equals_both_yardsticks(ctx, got, t):
    r = T.restate(t)
    assert not isinstance(r, str), r
    want, alone = ctx.font_create(r["leaf_off"], r["leaves"], r["bytes"]), ctx.font_create_tables(T.desc(t))
    try:
        a = ctx.font_read(got)
        for other in (want, alone):
            b = ctx.font_read(other)
            for k in ("leaf_off", "leaves", "bytes"):
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
                assert a[k].tobytes() == r[k].tobytes(), k
            assert got.device_bytes == other.device_bytes
    finally:
        want.free(), alone.free()
    return r


def built_equal(ctx, faces, expect=None, **kw):
    """one call over `faces` (Tables, or a ready description); expect[i]: OK (built and equal to its yardsticks) or the status of
    a face that must come back without a font.  -> the restated arrays of the built faces"""
    expect = [OK] * len(faces) if expect is None else expect
    res = ctx.fonts_create_tables([f if isinstance(f, dict) else T.desc(f) for f in faces], **kw)
    assert len(res) == len(faces)
    out = []
    try:
        for i, ((font, status, needed), t, want) in enumerate(zip(res, faces, expect)):
            assert status == want, (i, status)
            if want != OK:
                assert font is None, i
                out.append(None)
                continue
            assert font is not None, i
            out.append(assert_equals_both_yardsticks(ctx, font, t))
    finally:
        for font, _, _ in res:
            if font is not None:
                font.free()
    return out


COUNTS = [1, 63, 64, 65, 128, 129]


@pytest.mark.parametrize("faces", [
    [T.count_font(n) for n in COUNTS],
    [T.count_font(n) for n in COUNTS[::-1]],
    [EMPTY] + [T.count_font(n) for n in COUNTS],
    [T.count_font(n) for n in COUNTS] + [EMPTY],
    [T.count_font(65), EMPTY, T.count_font(63)],
    [T.count_font(64), EMPTY, EMPTY, T.count_font(129), EMPTY, EMPTY],
    [EMPTY, EMPTY, T.count_font(1), EMPTY, T.count_font(128), EMPTY],
    [T.count_font(64), T.count_font(1)],
    [EMPTY],
    [EMPTY, EMPTY],
], ids=["ascending", "descending", "empty_first", "empty_last", "empty_between", "two_empty_in_a_row", "empty_everywhere",
        "a_face_ends_on_a_workgroups_edge", "one_empty_face", "only_empty_faces"])
def test_every_workgroup_finds_its_face(ctx, faces):
    rs = built_equal(ctx, faces)
    for t, r in zip(faces, rs):
        assert len(r["leaf_off"]) == t.num_glyphs + 1        # (a face of 0 glyph ids has its one-entry leaf_off)


def test_unlike_neighbours_in_one_launch(ctx):
    faces = [T.forest_of(T.LONG_CASES).tables()]
    faces += [T.LOCA_FONTS[name] for name in sorted(T.LOCA_FONTS)]
    faces += [T.count_font(129, 64), T.count_font(65, None, "composite"), T.forest_of(T.LONG_CASES, -1).tables()]
    assert {t.loca_long for t in faces} == {0, 1}                  # short and long loca side by side
    rs = built_equal(ctx, faces)
    assert rs[-3]["leaf_off"][65] - rs[-3]["leaf_off"][64] == 32   # the deep glyph on a wave's first lane
    assert len(rs[-2]["leaves"]) == 0 and len(rs[-2]["bytes"]) == 0


def test_a_composite_cannot_reach_into_its_neighbour(ctx):
    """face A's composite names glyph id 5, which only face B has: skipped as in A alone, and nothing of B in A's leaves"""
    a = T.Forest()
    a.add("leafA", T.LEAF_A), a.add("leafB", T.LEAF_B)
    a.add("top", T.comp([T.rec("leafA"), T.rec(5), T.rec("leafB")]))
    b = T.Forest()
    for i in range(8):
        b.add(f"g{i}", T.simple(3 + i, seed=i))
    ta, tb = a.tables(), b.tables()
    ra = T.restate(ta)
    assert ra["leaf_off"][3] - ra["leaf_off"][2] == 2              # the two children A has
    for faces in ([ta, tb], [tb, ta], [tb, ta, tb]):
        built_equal(ctx, faces)


@pytest.mark.parametrize("bad,status", [(T.slots_font(1024), E_GLYF), (T.budget_font(1), E_GLYF),
                                        (dict(T.desc(T.case_tables("compose_three_levels")), loca_long=2), E_ARG)],
                         ids=["slot_bound", "component_budget", "loca_long_2"])
def test_a_refusal_does_not_spread(ctx, bad, status):
    good = [T.count_font(65), T.case_tables("compose_three_levels"), T.count_font(129, 64)]
    # the refused face first, between good faces, and last, in one call
    built_equal(ctx, [bad, good[0], bad, good[1], good[2], bad], [status, OK, status, OK, OK, status])


def test_both_refusals_and_a_bad_description_in_one_call(ctx):
    good = T.count_font(63)
    faces = [T.slots_font(1024), good, T.budget_font(1), dict(T.desc(good), num_glyphs=65536), good, dict(T.desc(good), loca_long=2)]
    built_equal(ctx, faces, [E_GLYF, OK, E_GLYF, E_ARG, OK, E_ARG])


def test_the_limit_is_taken_face_by_face(ctx):
    faces = [T.count_font(63), T.forest_of(T.LONG_CASES).tables(), T.count_font(65)]
    sizes = [store_bytes(T.restate(t)) for t in faces]
    assert sizes[1] > sizes[2]
    descs = [T.desc(t) for t in faces]
    res = ctx.fonts_create_tables(descs, max_store_bytes=sizes[0] + sizes[2])
    assert [s for _, s, _ in res] == [OK, OK, OK] and [n for _, _, n in res] == sizes
    assert res[0][0] is not None and res[1][0] is None and res[2][0] is not None     # face 1 is passed over, face 2 is not
    for i in (0, 2):
        assert_equals_both_yardsticks(ctx, res[i][0], faces[i])
        assert res[i][0].device_bytes >= sizes[i]
        res[i][0].free()
    res = ctx.fonts_create_tables(descs, max_store_bytes=sizes[0] - 1)
    assert [f for f, _, _ in res] == [None, None, None] and [s for _, s, _ in res] == [OK, OK, OK] and [n for _, _, n in res] == sizes
    res = ctx.fonts_create_tables(descs, max_store_bytes=sum(sizes))
    assert all(f is not None for f, _, _ in res) and [n for _, _, n in res] == sizes
    for f, _, _ in res:
        f.free()


def test_whole_call_arguments(vg, ctx):
    good = [T.count_font(65), T.case_tables("compose_three_levels")]

    def fails(descs, **kw):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.fonts_create_tables(descs, **kw)
        assert e.value.code == E_ARG, str(e.value)
        built_equal(ctx, good)                                   # the context is sound: a good batch behind every failure

    for name in ("faces", "out", "status"):
        fails([T.desc(t) for t in good], null=[name])
    nothing = {"loca": b"", "glyf": b"", "num_glyphs": 0, "loca_entries": 0, "loca_long": 1}      # descriptions only
    fails([nothing] * 65537)
    built_equal(ctx, [EMPTY] * 3)
    many = dict(nothing, num_glyphs=65535)
    assert 65 * 65535 > 1 << 22 >= 64 * 65535
    fails([many] * 65)
    assert ctx.fonts_create_tables([]) == []
    assert ctx.fonts_create_tables([T.desc(good[0])], n_faces=0, null=["faces", "out", "status"]) == []
    built_equal(ctx, [good[1]])                                  # a batch of one equals the single call


def test_submissions_over_the_fonts_of_one_batch(ctx):
    """one submit_resident that names several fonts and one ranges submission over a family of them, against the same over the
    yardstick fonts"""
    faces = [T.count_font(129, 64), T.count_font(65), T.case_tables("compose_three_levels")]
    rs = [T.restate(t) for t in faces]
    batch = [f for f, _, _ in ctx.fonts_create_tables([T.desc(t) for t in faces])]
    yard = [ctx.font_create(r["leaf_off"], r["leaves"], r["bytes"]) for r in rs]
    font_of, ids = [], []
    for k, r in enumerate(rs):
        for g in range(len(r["leaf_off"]) - 1):
            if r["leaf_off"][g + 1] > r["leaf_off"][g]:
                font_of.append(k), ids.append(g)
    font_of, ids = np.array(font_of[::-1] + [0, 0], dtype=np.uint16), np.array(ids[::-1] + [64, 64], dtype=np.uint16)
    n = len(ids)
    scale, shift = np.full(n, 24.0 / 1000.0), np.linspace(-0.4, 0.4, n)
    m = 129 + 65
    fam_font = np.concatenate([np.zeros(129, np.uint16), np.ones(65, np.uint16)])
    fam_gid = np.concatenate([np.arange(129), np.arange(65)])
    out = []
    for fonts in (batch, yard):
        assert all(f is not None for f in fonts)
        ctx.outlines_submit_resident(fonts, font_of, ids, scale, shift, capacity=1 << 24)
        rects, bitmaps, out_bytes, n_seg = ctx.outlines_wait()
        fam = ctx.family_create(fonts[:2], 0x41 + np.arange(m), fam_font, fam_gid, np.full(m, 17), np.full(m, 24.0 / 1000.0), np.linspace(-0.3, 0.3, m))
        ctx.outlines_submit_ranges([fam], [0, 0], [0x41, 0xC0], [0xBF, 0x1FF], capacity=1 << 22)
        rects2, bitmaps2, out_bytes2, n_seg2 = ctx.outlines_wait()
        fam.free()
        assert bitmaps is not None and bitmaps2 is not None and out_bytes > 0 and out_bytes2 > 0
        out.append((rects.tobytes(), bitmaps.tobytes(), out_bytes, n_seg, rects2.tobytes(), bitmaps2.tobytes(), out_bytes2, n_seg2))
    assert out[0] == out[1]
    for f in batch + yard:
        f.free()


def test_the_passes_are_timed(ctx):
    assert ctx.fonts_create_tables([]) == [] and ctx.fonts_tables_kernel_ms() == (0.0, 0.0)
    res = ctx.fonts_create_tables([T.desc(T.count_font(129)), T.desc(T.count_font(65))])
    ms = ctx.fonts_tables_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0
    for f, _, _ in res:
        f.free()
