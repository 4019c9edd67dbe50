"""One placed `glyf` face at MANY positions in one device call (vgsdf_fonts_create_gvar) against the single call and the host.

Every font the batched call returns is read back (vgsdf_font_commands_read) and compared byte for byte — cmd_off, the 28-byte
records, the context bytes, and what they occupy — with two things: what vgsdf_font_create_gvar makes of the same tables at that
position alone, and the store vgsdf_font_create_commands makes of the host reader's command table there (the reads of
test_gpu_gvar_regimes.py::assert_device_equals_host).  A position the single call refuses must be refused by the batched call,
there and only there.

The faces: every hand-written table of tests/gvar_instances_kit.py with all five positions in one call; glyph counts at the wave
edges of the (glyph id, position) index times 1, 2 and 5 positions; faces whose points x positions pass one launch of the deltas
pass; the deltas budget; the budget form; the validation.  After every refusal or error a good call on the same context succeeds.

Two statements of the issue this file was written for cannot hold beside "a position's font is what the single call makes of
it", and are tested as the single call has them:
  - VGSDF_GVAR_MAX_DELTAS bounds tuples x points WHATEVER the tuples' scalars (include/vgsdf.h, csrc/gvar_limits.h), so a face one
    past it is refused by the single call at every position: the batched call refuses every position too, not "only the first";
  - all stores of one call have the same size, so a limit cannot be "enough for the first and third position but not the second"
    by size.  What is tested: a limit of two stores builds the first two of three positions and passes the third over, and, with
    the second position refused, builds the first and the third — a refused position takes no room."""
import struct

import numpy as np
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
import test_gpu_gvar_regimes as R  # noqa: E402  (its faces and reads; its tests are not collected from here)

pytestmark = pytest.mark.gpu

VGSDF_OK, VGSDF_E_ARG, VGSDF_E_GLYF = 0, -1, -4
MAX_POSITIONS = 64      # VGSDF_GVAR_MAX_POSITIONS


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def _store(ctx, font):
    r = ctx.font_commands_read(font)
    return r["cmd_off"].tobytes(), r["records"].tobytes(), r["context"].tobytes(), font.device_bytes


def _free(fonts):
    for f in fonts:
        if f is not None:
            f.free()


def assert_batch_equals_single_and_host(vg, ctx, font, positions, expect=None):
    """one batched call over `positions`; -> the list of booleans "built".  expect: that list, when the caller knows it"""
    described = [R._described(vg, font, list(c)) for c in positions]
    fonts, status, needed = ctx.fonts_create_gvar(described[0][0], positions)
    try:
        assert len(fonts) == len(status) == len(needed) == len(positions)
        built = [f is not None for f in fonts]
        for p, (desc, host) in enumerate(described):
            if expect is not None:
                assert built[p] == expect[p], (p, status)
            if not built[p]:
                assert status[p] == VGSDF_E_GLYF, (p, status)
                with pytest.raises(vg.VgsdfError) as e:
                    ctx.font_create_gvar(desc)
                assert e.value.code == VGSDF_E_GLYF, p
                continue
            assert status[p] == VGSDF_OK, (p, status)
            a = ctx.font_create_gvar(desc)
            b = ctx.font_create_commands(host["cmd_off"], host["dat_off"], host["kinds"], host["coords"])
            try:
                got, single, want = _store(ctx, fonts[p]), _store(ctx, a), _store(ctx, b)
                assert np.array_equal(np.frombuffer(want[0], np.uint32), host["cmd_off"])
                assert got == single, p
                assert got == want, p
            finally:
                a.free()
                b.free()
        return built
    finally:
        _free(fonts)


def _good_call(vg, ctx):
    """the context is sound: a good batched call and a good single call on it"""
    font = G.edge_faces()["inference"][0]
    assert assert_batch_equals_single_and_host(vg, ctx, font, [[16384], [5000]]) == [True, True]


@pytest.mark.parametrize("case", sorted(G.edge_faces()))
def test_every_hand_written_face_at_five_positions_in_one_call(vg, ctx, case):
    font, _ = G.edge_faces()[case]
    positions = [R._edge_coords(case, p) for p in G.EDGE_POSITIONS]
    # a glyph id whose data is malformed AT A POSITION (a tuple of scalar 0 is not read) refuses that position, and only that
    expect = [all(G.restate(font, c)["ok"]) for c in positions]
    assert_batch_equals_single_and_host(vg, ctx, font, positions, expect)
    if not all(expect):
        _good_call(vg, ctx)


@pytest.mark.parametrize("n_positions", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_wave_edges_of_the_pair_index(vg, ctx, n, n_positions):
    """n glyph ids x n_positions pairs, position fastest: a wave ends inside a glyph id's positions, or between two glyph ids.  The
    default position (all 0) is among them from 2 on, and with 5 one position is given twice"""
    positions = [[16384], [0], [5000], [-8192], [5000]][:n_positions]
    assert_batch_equals_single_and_host(vg, ctx, R._sized_face(n), positions, [True] * n_positions)


def test_a_position_given_twice_yields_two_fonts_that_are_freed_apart(vg, ctx):
    font = R._sized_face(65)
    desc, _ = R._described(vg, font, [5000])
    fonts, status, _ = ctx.fonts_create_gvar(desc, [[5000], [16384], [5000]])
    assert status == [VGSDF_OK] * 3 and all(f is not None for f in fonts)
    first = _store(ctx, fonts[0])
    assert first == _store(ctx, fonts[2]) and first != _store(ctx, fonts[1])
    fonts[0].free()
    assert _store(ctx, fonts[2]) == first           # the twin lives on: its own store
    _free(fonts[1:])


def _passing_face():
    """glyph ids: 0 a square, 1 of 59904 points with a subset tuple (inference over contours of 19968 points), 2 a small glyph
    with a subset tuple, 3 a composite of 2 and 0.  Own points (+ 4): 8, 59908, 16, 6"""
    big, n = R._long_entry(59904, 3), 59904
    square = G.simple_entry([[(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]])
    numbers = list(range(3, n, 7))
    entries = [square, big, G.simple_entry([G._polygon(12)]), G.composite_entry([(2, 100, 50, None), (0, -200, 0, (0.5, 0.25, -0.25, 0.75))])]
    datas = [G.glyph_variations([G.tuple_of([1, -2, 3, -4, 0, 0, 0, 0], [5, 6, -7, 8, 0, 0, 0, 0], peak=[G.ONE], points=None)]),
             G.glyph_variations([G.tuple_of(G._ramp(len(numbers), 5), G._ramp(len(numbers), 9), peak=[G.ONE], points=numbers)]),
             G.glyph_variations([G.tuple_of([30, -10, 4], [8, 40, -4], peak=[G.ONE], points=[1, 6, 13])]),
             G.glyph_variations([G.tuple_of([24, -36, 0, 0, 0, 0], [12, 60, 0, 0, 0, 0], peak=[G.ONE], points=None)])]
    return G.raw_font(entries, G.gvar_table(datas)), [8, n + 4, 16, 6]


@pytest.mark.parametrize("n_positions", [2, 3])
def test_points_times_positions_at_and_past_one_launch(vg, ctx, n_positions):
    """2 positions: glyph ids 0 and 1 share a launch with both positions (119832 point-positions), 2 and 3 the next.  3 positions:
    glyph id 0 goes alone with all three — the slice ends between two glyph ids —, glyph id 1 passes the bound with three
    positions and goes alone in runs of two and one — the slice ends between two positions of one glyph id"""
    font, own = _passing_face()
    assert (own[0] + own[1]) * 2 <= R.SLICE_POINTS < (own[0] + own[1]) * 3 and own[1] * 2 <= R.SLICE_POINTS < own[1] * 3
    positions = [[16384], [5000], [8192]][:n_positions]
    assert_batch_equals_single_and_host(vg, ctx, font, positions, [True] * n_positions)
    # a fresh context, whose scratch is grown by these very launches, gives the same stores
    fresh = vg.SdfContext(0)
    try:
        assert_batch_equals_single_and_host(vg, fresh, font, positions, [True] * n_positions)
        _good_call(vg, fresh)
    finally:
        fresh.close()


def test_the_large_face_at_two_positions(vg, ctx):
    """the sliced face of test_gpu_gvar_regimes.py: every glyph id of 59908 points goes with both positions, alone"""
    assert_batch_equals_single_and_host(vg, ctx, R._sliced_face(8), [[16384], [5000]], [True, True])


def test_the_deltas_budget_at_and_one_past_it(vg, ctx):
    """the bound is on tuples x points whatever the scalars (module docstring): at it both positions are built — at [8192] the
    last tuple's scalar is a half —, one past it both are refused, as the single call refuses each"""
    font, deltas = R._budget_face(252)
    assert deltas <= R.MAX_DELTAS < deltas + 4095
    assert_batch_equals_single_and_host(vg, ctx, font, [[16384], [8192]], [True, True])
    font, deltas = R._budget_face(253)
    assert deltas > R.MAX_DELTAS
    desc, _ = R._described(vg, font, [16384])
    fonts, status, needed = ctx.fonts_create_gvar(desc, [[16384], [8192]], max_store_bytes=1 << 40)
    assert fonts == [None, None] and status == [VGSDF_E_GLYF] * 2 and needed == [0, 0]
    assert "VGSDF_GVAR_MAX_DELTAS" in ctx.last_error()
    assert_batch_equals_single_and_host(vg, ctx, font, [[16384], [8192]], [False, False])
    _good_call(vg, ctx)


def test_the_budget_form(vg, ctx):
    desc, host = R._good(vg)
    want = 29 * len(host["kinds"]) + 4 * len(host["cmd_off"])
    three = [[16384], [5000], [8192]]
    for limit, built in ((0, 0), (want - 1, 0), (want, 1), (want + 1, 1), (2 * want, 2), (3 * want - 1, 2), (3 * want, 3)):
        fonts, status, needed = ctx.fonts_create_gvar(desc, three, max_store_bytes=limit)
        try:
            assert [f is not None for f in fonts] == [True] * built + [False] * (3 - built), limit
            assert status == [VGSDF_OK] * 3 and needed == [want] * 3, limit
            single = ctx.font_create_gvar(dict(desc, coords=three[0]))
            try:
                assert built == 0 or _store(ctx, fonts[0]) == _store(ctx, single)
            finally:
                single.free()
        finally:
            _free(fonts)
    # the second position refused (malformed there): it takes no room, a limit of two stores builds the first and the third
    font = G.edge_faces()["composites_malformed"][0]
    positions = [[-8192], [16384], [0]]
    assert [all(G.restate(font, p)["ok"]) for p in positions] == [True, False, True]
    desc, host = R._described(vg, font, positions[0])
    want = 29 * len(host["kinds"]) + 4 * len(host["cmd_off"])
    fonts, status, needed = ctx.fonts_create_gvar(desc, positions, max_store_bytes=2 * want)
    try:
        assert [f is not None for f in fonts] == [True, False, True]
        assert status == [VGSDF_OK, VGSDF_E_GLYF, VGSDF_OK] and needed == [want, 0, want]
    finally:
        _free(fonts)
    _good_call(vg, ctx)
    ms = ctx.fonts_gvar_kernel_ms()
    assert len(ms) == 3 and all(v > 0 for v in ms)


def _refused(vg, ctx, why, desc, positions, **override):
    with pytest.raises(vg.VgsdfError) as e:
        ctx.fonts_create_gvar(desc, positions, **override)
    assert e.value.code == VGSDF_E_ARG and why in str(e.value), str(e.value)
    _good_call(vg, ctx)


def test_calls_that_are_refused_whole(vg, ctx):
    desc, _ = R._good(vg)
    two = [[16384], [5000]]
    for null in ("desc", "gvar", "coords", "out", "status"):
        _refused(vg, ctx, "NULL argument", desc, two, null=[null])
    gvar = desc["gvar"]
    array_end = 20 + 4 * (desc["num_glyphs"] + 1)
    # everything the single call validates
    for bad, positions, why in ((dict(desc, gvar=b"\0\2" + gvar[2:]), two, "version"), (desc, [[0, 0], [1, 1]], "axisCount"),
                                (desc, [[0] * 65, [1] * 65], "1 .. 64"), (dict(desc, gvar=gvar[:19]), two, "header"),
                                (dict(desc, gvar=gvar[:array_end - 1]), two, "offset array"), (dict(desc, gvar=gvar[:array_end + 1]), two, "shared tuples"),
                                (dict(desc, loca_long=2), two, "loca_long"), (dict(desc, loca_entries=desc["loca_entries"] + 1), two, "loca entries"),
                                (dict(desc, num_glyphs=desc["num_glyphs"] - 1), two, "num_glyphs + 1")):
        _refused(vg, ctx, why, bad, positions)
    # the last glyph id's data leaves a gvar stated one byte shorter: malformed, at every position where its tuple is read
    fonts, status, _ = ctx.fonts_create_gvar(desc, two, gvar_len=len(gvar) - 1)
    assert fonts == [None, None] and status == [VGSDF_E_GLYF] * 2 and "malformed variation data" in ctx.last_error()
    _good_call(vg, ctx)


def test_the_number_of_positions_0_64_and_65(vg, ctx):
    desc, host = R._good(vg)
    many = [[16384 - 200 * p] for p in range(MAX_POSITIONS + 1)]
    _refused(vg, ctx, "more than 64 positions", desc, many)
    # none: VGSDF_OK and nothing touched, whatever else is passed
    assert ctx.fonts_create_gvar(desc, []) == ([], [], [])
    assert ctx.fonts_create_gvar(desc, many[:1], n_positions=0, null=["out", "status", "gvar", "coords"]) == ([], [], [])
    fonts, status, _ = ctx.fonts_create_gvar(desc, many[:MAX_POSITIONS])
    try:
        assert status == [VGSDF_OK] * MAX_POSITIONS and all(f is not None for f in fonts)
        stores = [_store(ctx, f) for f in fonts]
        assert len(set(stores)) == MAX_POSITIONS                # 64 positions, 64 different stores
        for p in (0, 31, 63):
            single = ctx.font_create_gvar(dict(desc, coords=many[p]))
            try:
                assert stores[p] == _store(ctx, single), p
            finally:
                single.free()
    finally:
        _free(fonts)
    _good_call(vg, ctx)
