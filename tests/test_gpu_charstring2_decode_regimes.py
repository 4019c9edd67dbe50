"""The device's CFF2 charstring decoder (vgsdf_font_create_charstrings2) against the kit's strict interpreter
(tests/charstring2_edge_programs.py, which tests/test_charstring2_desc_host.py holds against the host reader): for one
description and one array of blend factors, the command font the device decodes and the one vgsdf_font_create_commands makes from
the interpreter's commands are read back (vgsdf_font_commands_read) and compared byte for byte — cmd_off, the 28-byte records, the
context bytes, and what they occupy.  Every face is checked with the factors of the default position, the faces with blends
again with factors no default position produces (0.3, -0.75, 1/3 as f32, 1e-3, ...): the factors are data.

The faces: the operand stack at the edge of the LDS window (48 slots) and at its limit (513), blends astride the window's edge,
every rule of `blend` and `vsindex`, the ends of a glyph, glyph counts at the wave edges with unlike neighbours, the boundary
between two launches (16384 glyph ids each), the token budget, the validation of the description."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring2_edge_programs as K2  # noqa: E402

pytestmark = pytest.mark.gpu

VGSDF_E_ARG, VGSDF_E_GLYF = -1, -4


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def assert_device_equals_interpreter(ctx, desc, sets=None):
    """sets: other blend sets than the description's, given to the device and to the interpreter alike"""
    d = dict(desc, **sets) if sets is not None else desc
    want, ends = K2.expected_commands(d)
    a = ctx.font_create_charstrings2(d)
    b = ctx.font_create_commands(want["cmd_off"], want["dat_off"], want["kinds"], want["coords"])
    try:
        ra, rb = ctx.font_commands_read(a), ctx.font_commands_read(b)
        assert np.array_equal(rb["cmd_off"], want["cmd_off"])
        assert np.array_equal(ra["cmd_off"], rb["cmd_off"])
        assert ra["records"].tobytes() == rb["records"].tobytes()
        assert ra["context"].tobytes() == rb["context"].tobytes()
        assert a.device_bytes == b.device_bytes
        return want, ends
    finally:
        a.free()
        b.free()


def both_positions(ctx, desc):
    want, ends = assert_device_equals_interpreter(ctx, desc)
    for shift in (0, 3):
        alt, _ = assert_device_equals_interpreter(ctx, desc, K2.alt_sets(desc, shift))
    return want, ends, alt


GOOD = None


def _good():
    global GOOD
    if GOOD is None:
        GOOD = K2.sized_face(65).desc()
    return GOOD


def test_every_program_among_unlike_neighbours(ctx):
    face = K2.shared_face()
    want, ends, alt = both_positions(ctx, face.desc())
    assert len(want["kinds"]) > 2500 and alt["coords"].tobytes() != want["coords"].tobytes()
    by_name = dict(zip([n for n, _ in face.glyphs], ends))
    assert (by_name["stack_513"], by_name["stack_514"], by_name["blend_depth_10"], by_name["vsindex_unusable"]) == ("end", "fail", "end", "fail")
    rng = np.random.default_rng(11)
    for order in (rng.permutation(len(face.glyphs) - 1), np.arange(len(face.glyphs) - 1)[::-1]):
        d = K2.shared_face(order=order).desc()
        assert_device_equals_interpreter(ctx, d)
        assert_device_equals_interpreter(ctx, d, K2.alt_sets(d, 5))


def test_every_program_as_a_face_of_its_own(ctx):
    """(no neighbour's slots of the workspace or of LDS can stand in for the glyph's own)"""
    loc, glo = K2._shared_sets()
    for name, cs in K2._programs():
        d = K2.Face(name, [(".notdef", K2.NOTDEF), (name, cs)], glo, loc).desc()
        try:
            assert_device_equals_interpreter(ctx, d)
            if name.startswith(("blend", "vsindex", "stack")):
                assert_device_equals_interpreter(ctx, d, K2.alt_sets(d, 1))
        except AssertionError as e:
            raise AssertionError(name) from e


def test_without_set_0_no_glyph_delivers_anything(ctx):
    for face in (K2.set0_unusable_face(), K2.no_sets_face()):
        want, ends = assert_device_equals_interpreter(ctx, face.desc())
        assert len(want["kinds"]) == 0 and set(ends) == {"fail"}
    # set 0 usable again: the same programs deliver
    d = dict(K2.set0_unusable_face().desc(), set_ok=np.array([1, 1], np.uint8))
    want, ends = assert_device_equals_interpreter(ctx, d)
    assert ends == ["end"] * 3 and len(want["kinds"]) == 5
    # n_sets == 0 with the arrays left out altogether
    d = K2.no_sets_face().desc()
    f = ctx.font_create_charstrings2(dict(d, set_off=np.zeros(0, np.uint32)))
    assert len(ctx.font_commands_read(f)["records"]) == 0
    f.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_glyph_counts_at_the_wave_edges(ctx, n):
    """neighbours in one wave select different sets and reach different depths of the stack"""
    want, ends, _ = both_positions(ctx, K2.sized_face(n, deep_last=min(n, 3)).desc())
    assert n == 1 or ("fail" in ends and "end" in ends)          # (glyph id 0 pushes a 514th operand)


def test_the_boundary_between_two_launches(ctx):
    face = K2.chunk_face(16385)
    d = face.desc()
    want, ends = assert_device_equals_interpreter(ctx, d)
    assert ends == ["end"] * 16385 and len(want["kinds"]) == 16385 + 2 * 508
    assert_device_equals_interpreter(ctx, d, K2.alt_sets(d, 2))
    # exactly one launch, and the last glyph id of a first launch beside the first of a second
    for n in (16384,):
        assert_device_equals_interpreter(ctx, K2.chunk_face(n).desc())


def _refused(vg, ctx, code, desc, why="", **override):
    with pytest.raises(vg.VgsdfError) as e:
        ctx.font_create_charstrings2(desc, **override)
    assert e.value.code == code and why in str(e.value), str(e.value)
    assert_device_equals_interpreter(ctx, _good())          # the context is sound: a good face behind every refusal


def test_token_budget(vg, ctx):
    at, over = K2.budget_faces()
    want, ends = assert_device_equals_interpreter(ctx, at.desc())    # exactly the budget: decoded
    assert ends == ["end", "end"] and len(want["kinds"]) == 4
    _refused(vg, ctx, VGSDF_E_GLYF, over.desc(), why="VGSDF_CHARSTRING_MAX_TOKENS")   # one token more


def test_bad_descriptions_are_refused_before_anything_runs(vg, ctx):
    good = K2.shared_face().desc()

    def bent(key, index, value):
        d = {k: (None if v is None else v.copy()) for k, v in good.items()}
        d[key][index] = value
        return d
    n_bytes = len(good["bytes"])
    cases = [
        # what the version 1 entry point refuses
        bent("cs_off", 3, int(good["cs_off"][2]) - 1),               # not ascending
        bent("cs_off", -1, n_bytes + 4),                             # past bytes
        bent("gsubr_off", 0, int(good["gsubr_off"][1]) + 1),
        bent("gsubr_off", -1, n_bytes + 1),
        bent("lsubr_off", 7, 0),
        bent("lsubr_off", -1, 0xFFFFFFFF),
        bent("lsubr_first", 0, 1),
        # the blend sets
        bent("set_off", 0, 1),                                       # does not start at 0
        bent("set_off", 2, int(good["set_off"][1]) - 1),             # not ascending
        bent("set_off", -1, len(good["factors"]) + 1),               # ends past the factors
        bent("factors", 2, np.inf), bent("factors", 0, -np.inf), bent("factors", len(good["factors"]) - 1, np.nan),
    ]
    for d in cases:
        _refused(vg, ctx, VGSDF_E_ARG, d)
    for override in ({"n_glyph_ids": 0}, {"n_glyph_ids": 65537}, {"n_bytes": n_bytes - 1}, {"n_fds": 0}, {"n_fds": 2}, {"n_gsubrs": 65536},
                     {"n_sets": 65537}, {"n_factors": len(good["factors"]) - 1}):
        _refused(vg, ctx, VGSDF_E_ARG, good, **override)
    _refused(vg, ctx, VGSDF_E_ARG, dict(good, fd_of=np.zeros(len(good["cs_off"]) - 1, np.uint8)))      # fd_of must be NULL
    # a set of 65 factors; 64 pass
    for k, ok in ((64, True), (65, False)):
        d = dict(K2.sized_face(3).desc(), set_ok=np.array([1], np.uint8), set_off=np.array([0, k], np.uint32), factors=np.full(k, 0.5, np.float32))
        if ok:
            ctx.font_create_charstrings2(d).free()
        else:
            _refused(vg, ctx, VGSDF_E_ARG, d, why="64")
    # a set marked not usable is validated like any other
    d = bent("set_ok", 1, 0)
    assert_device_equals_interpreter(ctx, d)
    assert_device_equals_interpreter(ctx, good)


def test_a_limit_on_the_store_is_checked_before_it_is_allocated(ctx):
    d = K2.sized_face(65).desc()
    want, _ = K2.expected_commands(d)
    size_want = 29 * len(want["kinds"]) + 4 * len(want["cmd_off"])
    font, size = ctx.font_create_charstrings2(d, max_store_bytes=size_want - 1)
    assert font is None and size == size_want
    font, size = ctx.font_create_charstrings2(d, max_store_bytes=size_want)
    assert font is not None and size == size_want and font.device_bytes >= size_want
    font.free()
    assert_device_equals_interpreter(ctx, d)


def test_the_variable_fira_face_at_the_c_abi(vg, ctx):
    """the description of a real CFF2 face: against the host reader's command table at the default position, against the
    interpreter at factors of another"""
    from test_cff2_outlines import _variable_fira
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Fira CFF2", _variable_fira())
    d, host = mgr.charstring2_font_desc(fid, 0), mgr.command_font_desc(fid, 0)
    want, _ = assert_device_equals_interpreter(ctx, d)
    assert want["kinds"].tobytes() == host["kinds"].tobytes() and want["coords"].tobytes() == host["coords"].tobytes()
    assert np.array_equal(want["cmd_off"], host["cmd_off"]) and len(host["kinds"]) > 5000
    for factor in (0.3, -0.75, float(np.float32(1.0) / np.float32(3.0)), 1e-3):
        sets = dict(K2.blend_sets(d), factors=np.full(len(d["factors"]), factor, np.float32))
        alt, _ = assert_device_equals_interpreter(ctx, d, sets)
        assert alt["coords"].tobytes() != want["coords"].tobytes()
    ms = ctx.font_charstrings_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0
