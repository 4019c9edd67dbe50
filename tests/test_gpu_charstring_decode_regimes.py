"""The device's charstring decoder (vgsdf_font_create_charstrings) against the host reader: for one face, the command font the
device decodes from the charstrings and the one vgsdf_font_create_commands makes from the host's description are read back
(vgsdf_font_commands_read) and compared byte for byte — cmd_off, the 28-byte records, the context bytes, and what they occupy.
The faces are the kit's (tests/charstring_edge_programs.py): every program at an edge of the interpreter's rules, alone and
among unlike neighbours, the wave and prefix-sum edges of the glyph count, the bias steps, Font DICTs, the refusals."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring_edge_programs as K  # noqa: E402

pytestmark = pytest.mark.gpu

VGSDF_E_ARG, VGSDF_E_GLYF = -1, -4


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def _host(vg, font_bytes):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Face", font_bytes)
    return mgr.charstring_font_desc(fid, 0), mgr.command_font_desc(fid, 0)


def assert_device_equals_host(ctx, cs_desc, cmd_desc):
    a = ctx.font_create_charstrings(cs_desc)
    b = ctx.font_create_commands(cmd_desc["cmd_off"], cmd_desc["dat_off"], cmd_desc["kinds"], cmd_desc["coords"])
    try:
        ra, rb = ctx.font_commands_read(a), ctx.font_commands_read(b)
        assert np.array_equal(rb["cmd_off"], cmd_desc["cmd_off"])
        assert np.array_equal(ra["cmd_off"], rb["cmd_off"])
        assert ra["records"].tobytes() == rb["records"].tobytes()
        assert ra["context"].tobytes() == rb["context"].tobytes()
        assert a.device_bytes == b.device_bytes
        return len(rb["records"])
    finally:
        a.free()
        b.free()


GOOD = None


def _good(vg):
    global GOOD
    if GOOD is None:
        GOOD = _host(vg, K.sized_face(65).font())
    return GOOD


def test_every_program_among_unlike_neighbours(vg, ctx):
    face = K.shared_face()
    n_cmds = assert_device_equals_host(ctx, *_host(vg, face.font()))
    assert n_cmds > 400
    rng = np.random.default_rng(11)
    for seed_order in (rng.permutation(len(face.glyphs) - 1), np.arange(len(face.glyphs) - 1)[::-1]):
        assert_device_equals_host(ctx, *_host(vg, K.shared_face(order=seed_order).font()))


def test_every_program_as_a_face_of_its_own(vg, ctx):
    # (the shell and the subroutines are shared; the description is the host's of each font)
    for face in K.single_faces():
        try:
            assert_device_equals_host(ctx, *_host(vg, face.font()))
        except AssertionError as e:
            raise AssertionError(face.name) from e


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_glyph_counts_at_the_wave_edges(vg, ctx, n):
    assert_device_equals_host(ctx, *_host(vg, K.sized_face(n).font()))


def test_empty_charstrings_at_the_prefix_sum_edges(vg, ctx):
    for empty in ({0}, {128}, {0, 128}, set(range(0, 129, 2)), set(range(1, 129, 2)), set(range(129))):
        assert_device_equals_host(ctx, *_host(vg, K.sized_face(129, empty=empty).font()))


def test_one_long_charstring_among_short_ones(vg, ctx):
    assert assert_device_equals_host(ctx, *_host(vg, K.long_face().font())) > 800


@pytest.mark.parametrize("face", K.bias_faces() + [K.cid_face()], ids=lambda f: f.name)
def test_bias_steps_and_font_dicts(vg, ctx, face):
    cs, cmd = _host(vg, face.font())
    assert (cs["fd_of"] is not None) == (face.name == "cid")
    assert_device_equals_host(ctx, cs, cmd)


def test_the_fonttools_built_faces(vg, ctx):
    from fira_cff_kit import fira_as_cff
    assert assert_device_equals_host(ctx, *_host(vg, fira_as_cff(400))) > 5000


def _refused(vg, ctx, code, desc, why="", **override):
    with pytest.raises(vg.VgsdfError) as e:
        ctx.font_create_charstrings(desc, **override)
    assert e.value.code == code and why in str(e.value), str(e.value)
    assert_device_equals_host(ctx, *_good(vg))          # the context is sound: a good face behind every refusal


def test_refusals_leave_the_context_sound(vg, ctx):
    for face in K.seac_faces():
        _refused(vg, ctx, VGSDF_E_GLYF, _host(vg, face.font())[0], why="seac")
    at, over = K.budget_faces()
    assert_device_equals_host(ctx, *_host(vg, at.font()))            # exactly the budget: decoded
    _refused(vg, ctx, VGSDF_E_GLYF, _host(vg, over.font())[0], why="VGSDF_CHARSTRING_MAX_TOKENS")                   # one token more


def test_bad_descriptions_are_refused_before_anything_runs(vg, ctx):
    good = K.cid_face().desc()

    def bent(key, index, value):
        d = {k: (None if v is None else v.copy()) for k, v in good.items()}
        d[key][index] = value
        return d
    n_bytes = len(good["bytes"])
    cases = [
        bent("cs_off", 3, int(good["cs_off"][2]) - 1),               # not ascending
        bent("cs_off", -1, n_bytes + 4),                             # past bytes
        bent("gsubr_off", 0, int(good["gsubr_off"][1]) + 1),
        bent("gsubr_off", -1, n_bytes + 1),
        bent("lsubr_off", 7, 0),
        bent("lsubr_off", -1, 0xFFFFFFFF),
        bent("lsubr_first", 0, 1),
        bent("lsubr_first", 2, int(good["lsubr_first"][1]) - 1),
        bent("fd_of", 5, 3),                                         # n_fds == 3
        bent("fd_of", len(good["fd_of"]) - 1, 255),
    ]
    for d in cases:
        _refused(vg, ctx, VGSDF_E_ARG, d)
    for override in ({"n_glyph_ids": 0}, {"n_glyph_ids": 65537}, {"n_bytes": n_bytes - 1}, {"n_fds": 0}, {"n_fds": 257}, {"n_gsubrs": 65536}):
        _refused(vg, ctx, VGSDF_E_ARG, good, **override)
    no_fd = dict(good, fd_of=None)                                   # several Font DICTs and no fd_of
    _refused(vg, ctx, VGSDF_E_ARG, no_fd)
    assert_device_equals_host(ctx, *_host(vg, K.cid_face().font()))


def test_a_limit_on_the_store_is_checked_before_it_is_allocated(vg, ctx):
    cs, cmd = _host(vg, K.sized_face(65).font())
    want = 29 * len(cmd["kinds"]) + 4 * len(cmd["cmd_off"])
    font, size = ctx.font_create_charstrings(cs, max_store_bytes=want - 1)
    assert font is None and size == want
    font, size = ctx.font_create_charstrings(cs, max_store_bytes=want)
    assert font is not None and size == want and font.device_bytes >= want
    font.free()
    assert_device_equals_host(ctx, cs, cmd)
