"""Glyf fonts built on the device from `loca` and `glyf` (vgsdf_font_create_tables; csrc/glyf_table_kernels.hip) at the edges of
the composite walk and of the two passes: every hand-written tree of tests/composite_edge_trees.py alone and side by side, the
loca formats and damaged locas, glyph-id counts around the wave, the deep glyph on a wave's first and last lane, faces without a
simple glyph and without a composite, the component budget and the slot bound on either side, the store limit, bad
descriptions, and submissions over a device-built font.

The yardstick is vgsdf_font_create of the arrays the Python restatement gives for the same tables (pinned to the host reader by
tests/test_font_tables_desc_host.py); both fonts are read back with vgsdf_font_read and compared array by array, byte for byte,
with device_bytes.  No tolerance appears anywhere."""
import numpy as np
import pytest

import composite_edge_trees as T

pytestmark = pytest.mark.gpu

E_ARG, E_GLYF = -1, -4


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


def both_ways(ctx, t):
    """-> (the device-built font, its yardstick, the restated arrays)"""
    r = T.restate(t)
    assert not isinstance(r, str), r
    want = ctx.font_create(r["leaf_off"], r["leaves"], r["bytes"])
    got = ctx.font_create_tables(T.desc(t))
    return got, want, r


def assert_same_font(ctx, t):
    got, want, r = both_ways(ctx, t)
    try:
        a, b = ctx.font_read(got), ctx.font_read(want)
        for k in ("leaf_off", "leaves", "bytes"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
            assert a[k].tobytes() == r[k].tobytes(), k                      # (the yardstick holds what it was given)
        assert got.device_bytes == want.device_bytes
    finally:
        got.free(), want.free()
    return r


def refused(vg, ctx, code, d, why="", **override):
    with pytest.raises(vg.VgsdfError) as e:
        ctx.font_create_tables(d, **override)
    assert e.value.code == code and why in str(e.value), str(e.value)
    assert_same_font(ctx, T.case_tables("compose_three_levels"))           # the context is sound: a good face behind every refusal


@pytest.mark.parametrize("name", T.LONG_CASES)
def test_edge_case_alone(ctx, name):
    assert_same_font(ctx, T.case_tables(name))


@pytest.mark.parametrize("order", [1, -1])
def test_edge_cases_among_unlike_neighbours(ctx, order):
    assert_same_font(ctx, T.forest_of(T.LONG_CASES, order).tables())


@pytest.mark.parametrize("name", sorted(T.LOCA_FONTS))
def test_loca_fonts(ctx, name):
    assert_same_font(ctx, T.LOCA_FONTS[name])


@pytest.mark.parametrize("n,deep_at,kind", [(1, None, "mixed"), (63, None, "mixed"), (64, None, "mixed"), (65, None, "mixed"), (127, None, "mixed"),
                                            (128, None, "mixed"), (129, None, "mixed"),
                                            (64, 0, "mixed"), (64, 63, "mixed"), (129, 64, "mixed"), (129, 127, "mixed"), (129, 128, "mixed"),
                                            (65, None, "simple"), (65, None, "composite"), (1, None, "composite")])
def test_glyph_id_counts_and_the_deep_glyph_on_a_waves_edge(ctx, n, deep_at, kind):
    r = assert_same_font(ctx, T.count_font(n, deep_at, kind))
    if deep_at is not None:
        assert r["leaf_off"][deep_at + 1] - r["leaf_off"][deep_at] == 32
    if kind == "composite":
        assert len(r["leaves"]) == 0 and len(r["bytes"]) == 0


def test_the_component_budget_on_either_side(vg, ctx):
    r = assert_same_font(ctx, T.budget_font(0))                              # exactly the budget: built
    assert max(r["records"]) == T.MAX_COMPONENTS
    assert T.restate(T.budget_font(1)) == T.REFUSED_BUDGET
    refused(vg, ctx, E_GLYF, T.desc(T.budget_font(1)), why="VGSDF_GLYF_MAX_COMPONENTS")   # one record more


def test_the_slot_bound_on_either_side(vg, ctx):
    r = assert_same_font(ctx, T.slots_font(1023))
    assert int(r["slots"].max()) == 1023 * 65537
    assert T.restate(T.slots_font(1024)) == T.REFUSED_BOUNDS
    refused(vg, ctx, E_GLYF, T.desc(T.slots_font(1024)), why="2^26")


def test_the_leaf_bound_on_either_side(vg, ctx):
    r = assert_same_font(ctx, T.leaves_font(0))                              # exactly 2^22 leaves: built
    assert len(r["leaves"]) == T.MAX_LEAVES
    assert T.restate(T.leaves_font(1)) == T.REFUSED_BOUNDS
    refused(vg, ctx, E_GLYF, T.desc(T.leaves_font(1)), why="2^22 leaves")    # one leaf more


def test_bad_descriptions_are_refused_before_anything_runs(vg, ctx):
    t = T.case_tables("compose_three_levels")
    good = T.desc(t)
    refused(vg, ctx, E_ARG, dict(good, num_glyphs=65536))
    refused(vg, ctx, E_ARG, dict(good, loca_long=2))
    refused(vg, ctx, E_ARG, dict(good, loca_entries=len(t.loca) // 4 + 1))
    refused(vg, ctx, E_ARG, dict(good, loca_long=0, loca_entries=len(t.loca) // 2 + 1))
    refused(vg, ctx, E_ARG, dict(good, num_glyphs=t.num_glyphs - 1))                    # loca_entries past num_glyphs + 1
    refused(vg, ctx, E_ARG, dict(good, loca=b""), n_loca_bytes=len(t.loca))          # NULL beside a length
    refused(vg, ctx, E_ARG, dict(good, glyf=b""), n_glyf_bytes=len(t.glyf))
    cmd = ctx.font_create_commands([0, 1], [0, 0], [4], [])
    with pytest.raises(vg.VgsdfError) as e:                                            # a command font has no leaves to read
        ctx.font_read(cmd)
    assert e.value.code == E_ARG
    cmd.free()


def test_a_limit_on_the_store_is_checked_before_it_is_allocated(ctx):
    t = T.forest_of(T.LONG_CASES).tables()
    r = T.restate(t)
    want = (48 * len(r["leaves"]) + len(r["bytes"]) + 15) // 16 * 16 + 4 * len(r["leaf_off"])
    font, size = ctx.font_create_tables(T.desc(t), max_store_bytes=want - 1)
    assert font is None and size == want
    font, size = ctx.font_create_tables(T.desc(t), max_store_bytes=want)
    assert font is not None and size == want and font.device_bytes >= want
    font.free()
    ms = ctx.font_tables_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0


def test_submissions_over_a_device_built_font(ctx):
    """one submit_resident and one ranges submission over the device-built font against the same over the yardstick"""
    t = T.count_font(129, 64)
    got, want, r = both_ways(ctx, t)
    ids = np.array([g for g in range(129) if r["leaf_off"][g + 1] > r["leaf_off"][g]] + [4, 64, 64], dtype=np.uint16)
    n = len(ids)
    scale, shift = np.full(n, 24.0 / 1000.0), np.linspace(-0.4, 0.4, n)
    out = []
    for font in (got, want):
        ctx.outlines_submit_resident([font], np.zeros(n, np.uint16), ids, scale, shift, capacity=1 << 22)
        rects, bitmaps, out_bytes, n_seg = ctx.outlines_wait()
        fam = ctx.family_create([font], 0x41 + np.arange(129), np.zeros(129, np.uint16), np.arange(129), np.full(129, 17), np.full(129, 24.0 / 1000.0),
                                np.linspace(-0.3, 0.3, 129))
        ctx.outlines_submit_ranges([fam], [0, 0], [0x41, 0x80], [0x7F, 0xFF], capacity=1 << 22)
        rects2, bitmaps2, out_bytes2, n_seg2 = ctx.outlines_wait()
        fam.free()
        assert bitmaps is not None and bitmaps2 is not None and out_bytes > 0 and out_bytes2 > 0
        out.append((rects.tobytes(), bitmaps.tobytes(), out_bytes, n_seg, rects2.tobytes(), bitmaps2.tobytes(), out_bytes2, n_seg2))
    assert out[0] == out[1]
    got.free(), want.free()
