"""The two store layouts of resident fonts (csrc/upload_layout.h: GlyfStoreLayout, CommandStoreLayout) where a constructor could
be wired to them wrongly: the same tiny face built by both constructors of its kind and read back — every array byte for byte,
and device_bytes.

Glyf kind (vgsdf_font_create of the restated arrays against vgsdf_font_create_tables): simple-entry bytes that end 0, 4, 8 and 12
past a multiple of 16 (the padding in front of leaf_off), a face without a leaf, and no glyph id at all.  Command kind
(vgsdf_font_create_commands of the host reader's table against vgsdf_font_create_charstrings): 1 and 65 glyph ids with the command
count 0 .. 3 past a multiple of 4 (cmd_off and the context bytes lie behind the 28-byte records), a face of bare `endchar`s (no
command: the emit pass is skipped), and the store limit one below and exactly at the store's size.  Families of 0 and 1 entries
by both constructors are tests/test_gpu_family_tables_regimes.py's entries_0 and entries_1.  No tolerance appears anywhere."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring_edge_programs as K  # noqa: E402
import composite_edge_trees as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


# ---- glyf kind ----

def glyf_face(trailing):
    """six glyph ids: two leaves, a composite of both, an empty range, a glyph without contours, and a simple glyph with
    `trailing` bytes behind its arrays (they are stored with it)"""
    f = T.Forest()
    f.add("leafA", T.LEAF_A), f.add("leafB", T.LEAF_B)
    f.add("both", T.comp([T.rec("leafA", T.ARGS_XY, T.xy(3, -2, False)), T.rec("leafB", T.ARGS_XY | T.SCALE, T.xy(1, 1, False) + T.f2(0.5))]))
    f.add("empty", b""), f.add("no_contours", b"\0\0")
    f.add("tail", T.simple(6, trailing=bytes(range(1, trailing + 1))))
    return f.tables()


def glyf_faces_by_residue():
    """residue of the stored bytes mod 16 -> Tables, for 0, 4, 8 and 12"""
    out = {}
    for trailing in range(16):
        t = glyf_face(trailing)
        out.setdefault(len(T.restate(t)["bytes"]) % 16, t)
    assert sorted(out) == [0, 4, 8, 12]
    return out


GLYF_FACES = glyf_faces_by_residue()
NO_LEAF = T.pack([b"", b"\0\0", T.comp([T.rec(0xFFFF)])(None), b"", b""])       # five glyph ids, none delivers anything
NO_GLYPH_ID = T.pack([])


def assert_same_glyf_font(ctx, t):
    r = T.restate(t)
    assert not isinstance(r, str), r
    want, got = ctx.font_create(r["leaf_off"], r["leaves"], r["bytes"]), ctx.font_create_tables(T.desc(t))
    try:
        a, b = ctx.font_read(got), ctx.font_read(want)
        for k in ("leaf_off", "leaves", "bytes"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() == r[k].tobytes(), k
        assert got.device_bytes == want.device_bytes
    finally:
        got.free(), want.free()
    return r


@pytest.mark.parametrize("residue", [0, 4, 8, 12])
def test_glyf_stores_with_every_padding_in_front_of_leaf_off(ctx, residue):
    r = assert_same_glyf_font(ctx, GLYF_FACES[residue])
    assert len(r["bytes"]) % 16 == residue and len(r["leaf_off"]) == 7 and len(r["leaves"]) == 5


def test_glyf_stores_without_a_leaf_and_without_a_glyph_id(ctx):
    r = assert_same_glyf_font(ctx, NO_LEAF)
    assert len(r["leaf_off"]) == 6 and len(r["leaves"]) == 0 and len(r["bytes"]) == 0
    r = assert_same_glyf_font(ctx, NO_GLYPH_ID)                                 # num_glyphs = 0 against n_glyph_ids = 0
    assert r["leaf_off"].tolist() == [0] and len(r["leaves"]) == 0 and len(r["bytes"]) == 0


# ---- command kind ----

def command_face(n, lines):
    """K.sized_face(n) with `lines` more line commands in its last glyph"""
    face = K.sized_face(n)
    name, cs = face.glyphs[-1]
    assert cs.endswith(K.enc("endchar"))
    face.glyphs[-1] = (name, cs[:-len(K.enc("endchar"))] + K.enc(*([3, -2] * lines), "rlineto", "endchar") if lines else cs)
    return face


def bare_face(n):
    return K.Face(f"bare_{n}", [(f"g{g}", K.enc("endchar")) for g in range(n)])


def host_descs(vg, face):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Face", face.font())
    return mgr.charstring_font_desc(fid, 0), mgr.command_font_desc(fid, 0)


def assert_same_command_font(ctx, cs, cmd, **within):
    """-> (commands, what font_create_charstrings returned beside the font)"""
    a = ctx.font_create_charstrings(cs, **within)
    size = None
    if within:
        a, size = a
        assert a is not None
    b = ctx.font_create_commands(cmd["cmd_off"], cmd["dat_off"], cmd["kinds"], cmd["coords"])
    try:
        ra, rb = ctx.font_commands_read(a), ctx.font_commands_read(b)
        assert ra["cmd_off"].tobytes() == rb["cmd_off"].tobytes() == np.asarray(cmd["cmd_off"], np.uint32).tobytes()
        assert ra["records"].tobytes() == rb["records"].tobytes() and len(rb["records"]) == len(cmd["kinds"])
        assert ra["context"].tobytes() == rb["context"].tobytes() and len(rb["context"]) == len(cmd["kinds"])
        assert a.device_bytes == b.device_bytes
    finally:
        a.free(), b.free()
    return len(cmd["kinds"]), size


@pytest.mark.parametrize("n", [1, 65])
def test_command_stores_with_every_command_count_mod_4(vg, ctx, n):
    seen = set()
    for lines in range(4):
        n_cmds, _ = assert_same_command_font(ctx, *host_descs(vg, command_face(n, lines)))
        ms = ctx.font_charstrings_kernel_ms()
        assert n_cmds > 0 and ms[0] > 0 and ms[1] > 0
        seen.add(n_cmds % 4)
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("n", [1, 65])
def test_a_face_without_a_command_skips_the_emit_pass(vg, ctx, n):
    cs, cmd = host_descs(vg, bare_face(n))
    assert len(cmd["kinds"]) == 0 and len(cmd["coords"]) == 0
    n_cmds, _ = assert_same_command_font(ctx, cs, cmd)
    ms = ctx.font_charstrings_kernel_ms()
    assert n_cmds == 0 and ms[0] > 0 and ms[1] == 0


def test_the_store_limit_one_below_and_at_the_stores_size(vg, ctx):
    cs, cmd = host_descs(vg, command_face(65, 1))
    want = 29 * len(cmd["kinds"]) + 4 * len(cmd["cmd_off"])
    font, size = ctx.font_create_charstrings(cs, max_store_bytes=want - 1)
    assert font is None and size == want                                        # (the call itself returned VGSDF_OK)
    _, size = assert_same_command_font(ctx, cs, cmd, max_store_bytes=want)
    assert size == want
