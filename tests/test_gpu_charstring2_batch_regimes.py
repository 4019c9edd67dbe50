"""vgsdf_fonts_create_charstrings2: one CFF2 face at many positions in one device build, at the C ABI.

The statement under test has two parts, and no tolerance: store p of the batched call equals, byte for byte (cmd_off, the 28-byte
records and the context bytes through vgsdf_font_commands_read, and vgsdf_font_device_bytes), the store the single call
vgsdf_font_create_charstrings2 makes at position p's factors; and both equal the store vgsdf_font_create_commands makes of the
strict interpreter's commands under those factors (tests/charstring2_edge_programs.py, tests/charstring2_batch_kit.py).

The regimes: every kit program at 1, 3 and 9 positions; pair counts at the wave edges, with one glyph id's positions astride two
waves; the operand stack astride the LDS window with factors that differ per position (a wrong workspace column would show one
position's operands in another's store); the edge between two launches (16384 lanes); programs whose control flow depends on the
position, so that the stores of one call have different sizes; refusals of one position and of all; the budget form; validation."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring2_batch_kit as B  # noqa: E402
import charstring2_edge_programs as K2  # noqa: E402

pytestmark = pytest.mark.gpu

OK, E_ARG, E_GLYF = B.VGSDF_OK, B.VGSDF_E_ARG, B.VGSDF_E_GLYF


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shared(ctx):
    """the face of every kit program and its yardsticks per position: made once, shared, never changed"""
    d = K2.shared_face().desc()
    return d, B.Yardsticks(ctx, d)


def _f(*v):
    return np.array(v, np.float32)


@pytest.mark.parametrize("n_pos", [1, 3, 9])
def test_every_kit_program_at_several_positions(ctx, shared, n_pos):
    d, y = shared
    positions = B.positions_of(d, n_pos)
    got = B.assert_batch_equals_single_and_interpreter(ctx, d, positions, y)
    assert len(d["cs_off"]) - 1 > 150 and len(got[0][0]["kinds"]) > 2500
    if n_pos >= 3:
        assert positions[-1].tobytes() == positions[1].tobytes()                         # the same position twice: two fonts
        assert got[0][0]["coords"].tobytes() != got[1][0]["coords"].tobytes()            # ... and the positions are positions
    ms = ctx.fonts_charstrings2_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0


@pytest.mark.parametrize("n,n_pos", [(1, 1), (21, 3), (64, 1), (65, 1), (22, 3), (43, 3), (129, 1), (7, 9), (8, 9)],
                         ids=lambda v: str(v))
def test_pair_counts_at_the_wave_edges(ctx, n, n_pos):
    """1, 63, 64, 65, 66, 129 (and 63, 72) pairs; with 22 glyph ids x 3 and 8 x 9 one glyph id's positions lie astride two waves.
    Neighbouring glyph ids select different sets and reach different depths of the stack, neighbouring positions have different
    factors"""
    d = K2.sized_face(n, deep_last=min(n, 3)).desc()
    got = B.assert_batch_equals_single_and_interpreter(ctx, d, B.positions_of(d, n_pos, twice=False))
    assert n == 1 or ("fail" in got[0][1] and "end" in got[0][1])                        # (glyph id 0 pushes a 514th operand)
    if n_pos > 1:
        assert got[0][0]["coords"].tobytes() != got[1][0]["coords"].tobytes()


def test_the_operand_stack_astride_the_lds_window_per_pair(ctx):
    face = B.window_face()
    d = face.desc()
    positions = B.positions_of(d, 3, twice=False)
    got = B.assert_batch_equals_single_and_interpreter(ctx, d, positions)
    by_name = dict(zip([n for n, _ in face.glyphs], got[0][1]))
    assert (by_name["stack_47"], by_name["stack_48"], by_name["stack_49"], by_name["stack_512"], by_name["stack_513"],
            by_name["stack_514"]) == ("end",) * 5 + ("fail",)
    # the blends' results differ per position: a store holding another position's operands would differ from its single call
    assert len({w["coords"].tobytes() for w, _ in got}) == 3


@pytest.mark.parametrize("n,n_pos,deep", [(5462, 3, (5460, 5461)), (16385, 1, (16383, 16384)), (257, 64, (255, 256))],
                         ids=["5462x3", "16385x1", "257x64"])
def test_the_edge_between_two_launches(ctx, n, n_pos, deep):
    """16386 pairs in launches of 5461 glyph ids x 3 (the last launch: one glyph id); 16385 x 1; 64 positions, 256 glyph ids per
    launch.  The glyph ids on either side of the edge fill the whole operand stack"""
    d = B.launch_edge_face(n, deep).desc()
    base = B.positions_of(d, 4, twice=False)
    positions = [base[p % 4] for p in range(n_pos)]                                      # (64 positions: four distinct ones, cycled)
    got = B.assert_batch_equals_single_and_interpreter(ctx, d, positions)
    assert got[0][1] == ["end"] * n and len(got[0][0]["kinds"]) == n + 2 * 508
    if n_pos > 1:
        assert got[0][0]["coords"].tobytes() != got[1][0]["coords"].tobytes()


def test_programs_whose_control_flow_depends_on_the_position(ctx):
    """(tests/test_charstring2_batch_desc_host.py shows on the host that the counts differ.)  The position at which two glyphs
    fail, f = 0.3, stands between positions at which they succeed"""
    face = B.position_dependent_face()
    d = face.desc()
    positions = [_f(0.0), _f(1.0), _f(0.3), _f(0.5), _f(1.0), _f(0.0)]
    got = B.assert_batch_equals_single_and_interpreter(ctx, d, positions)
    sizes = [B.store_bytes_of(w) for w, _ in got]
    assert len(set(sizes)) >= 3 and sizes[0] != sizes[1]                                  # stores of different sizes in one call
    g_of = {n: g for g, (n, _) in enumerate(face.glyphs)}
    for name in B.POSITION_DEPENDENT:
        g = g_of[name]
        for (want, ends), f in zip(got, (0.0, 1.0, 0.3, 0.5, 1.0, 0.0)):
            lines = B.LINES_AT[name][f]
            assert int(want["cmd_off"][g + 1]) - int(want["cmd_off"][g]) == (1 if lines is None else 1 + lines), (name, f)
            assert ends[g] == ("fail" if lines is None else "end")
    fonts, status, needed = ctx.fonts_create_charstrings2(d, positions, max_store_bytes=1 << 40)
    assert needed == sizes and status == [OK] * 6
    for f in fonts:
        f.free()


def test_a_position_independent_face_past_the_budget_refuses_every_position(vg, ctx):
    """(a glyph exactly at the budget is decoded: f = 0 of the test below)"""
    _, over = K2.budget_faces()
    d = over.desc()
    fonts, status, needed = ctx.fonts_create_charstrings2(d, B.positions_of(d, 3), max_store_bytes=1 << 40)
    assert fonts == [None] * 3 and status == [E_GLYF] * 3 and needed == [0] * 3
    with pytest.raises(vg.VgsdfError) as e:
        ctx.font_create_charstrings2(d)                                                    # as the single call
    assert e.value.code == E_GLYF


def test_a_position_past_the_budget_is_refused_alone(vg, ctx):
    """the blended subroutine index selects the long subroutine at f = 1 only: that position is refused, its neighbours —
    exactly at the budget at f = 0, failing at once at f = 0.3 — are built"""
    d = B.budget_by_position_face().desc()
    positions = [_f(0.0), _f(1.0), _f(0.3), _f(0.0)]
    fonts, status, needed = ctx.fonts_create_charstrings2(d, positions, max_store_bytes=1 << 40)
    try:
        assert status == [OK, E_GLYF, OK, OK] and fonts[1] is None and needed[1] == 0
        y = B.Yardsticks(ctx, d)
        for p in (0, 2, 3):
            single, kit, want, ends = y.at(positions[p])
            assert B.read_store(ctx, fonts[p]) == single == kit and needed[p] == B.store_bytes_of(want)
            assert ends[2] == ("end" if p != 2 else "fail") and len(want["kinds"]) == (6 if p != 2 else 3)
        with pytest.raises(vg.VgsdfError) as e:
            ctx.font_create_charstrings2(dict(d, factors=positions[1]))
        assert e.value.code == E_GLYF and "VGSDF_CHARSTRING_MAX_TOKENS" in str(e.value)
    finally:
        for f in fonts:
            if f is not None:
                f.free()


def test_without_set_0_every_store_is_empty(ctx):
    for face in (K2.set0_unusable_face(), K2.no_sets_face()):
        d = face.desc()
        got = B.assert_batch_equals_single_and_interpreter(ctx, d, B.positions_of(d, 3))
        assert all(len(w["kinds"]) == 0 and set(ends) == {"fail"} for w, ends in got)


def test_a_limit_takes_the_positions_in_order(ctx):
    """the stores of the position-dependent face have different sizes: the middle one is the largest"""
    d = B.position_dependent_face().desc()
    positions = [_f(0.0), _f(1.0), _f(0.5)]
    y = B.Yardsticks(ctx, d)
    sizes = [B.store_bytes_of(y.at(p)[2]) for p in positions]
    assert sizes[1] > sizes[0] > sizes[2]

    def within(limit, built):
        fonts, status, needed = ctx.fonts_create_charstrings2(d, positions, max_store_bytes=limit)
        try:
            assert status == [OK] * 3 and needed == sizes                                 # the single calls' store_bytes
            assert [f is not None for f in fonts] == built, limit
            for p, f in enumerate(fonts):
                if f is not None:
                    assert B.read_store(ctx, f) == y.at(positions[p])[0] and f.device_bytes >= sizes[p]
        finally:
            for f in fonts:
                if f is not None:
                    f.free()
    for p, factors in enumerate(positions):                                                # (what the single call says it needs)
        font, size = ctx.font_create_charstrings2(dict(d, factors=factors), max_store_bytes=0)
        assert font is None and size == sizes[p]
    within(sizes[2] - 1, [False, False, False])                                            # room for none
    within(sizes[0], [True, False, False])                                                 # for the first only
    within(sizes[0] + sizes[2], [True, False, True])                                       # one that does not fit is passed over
    within(sizes[0] + sizes[1] - 1, [True, False, True])
    within(sum(sizes), [True, True, True])


def test_bad_calls_are_refused_before_anything_runs(vg, ctx, shared):
    good, y = shared
    positions = B.positions_of(good, 3)

    def refused(desc, ps, why="", **override):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.fonts_create_charstrings2(desc, ps, **override)                            # (asserts that no font is left behind)
        assert e.value.code == E_ARG and why in str(e.value), str(e.value)
        B.assert_batch_equals_single_and_interpreter(ctx, good, positions[:2], y)          # the context is sound

    def bent(key, index, value):
        d = {k: (None if v is None else v.copy()) for k, v in good.items()}
        d[key][index] = value
        return d
    for null in ("desc", "out", "status", "factors"):
        refused(good, positions, why="NULL", null=(null,))
    refused(good, [positions[p % 3] for p in range(65)], why="64 positions")
    ctx.fonts_create_charstrings2(good, [positions[p % 3] for p in range(65)], n_positions=0)     # no position: nothing is touched
    assert ctx.fonts_create_charstrings2(good, [], null=("out", "status")) == ([], [], [])
    n_bytes = len(good["bytes"])
    # what the single call validates
    for d in (bent("cs_off", 3, int(good["cs_off"][2]) - 1), bent("cs_off", -1, n_bytes + 4), bent("gsubr_off", -1, n_bytes + 1),
              bent("lsubr_off", 7, 0), bent("lsubr_first", 0, 1), bent("set_off", 0, 1), bent("set_off", 2, int(good["set_off"][1]) - 1),
              bent("set_off", -1, len(good["factors"]) + 1), dict(good, fd_of=np.zeros(len(good["cs_off"]) - 1, np.uint8))):
        refused(d, positions)
    for override in ({"n_glyph_ids": 0}, {"n_glyph_ids": 65537}, {"n_bytes": n_bytes - 1}, {"n_fds": 0}, {"n_fds": 2}, {"n_gsubrs": 65536},
                     {"n_sets": 65537}, {"n_factors": len(good["factors"]) - 1}):
        refused(good, positions, **override)
    # a factor that is not finite, at any position
    for p, i, v in ((0, 0, np.inf), (1, 5, -np.inf), (2, len(good["factors"]) - 1, np.nan)):
        ps = [f.copy() for f in positions]
        ps[p][i] = v
        refused(good, ps, why="finite")
