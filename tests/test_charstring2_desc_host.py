"""The host half of CFF2 charstrings on the device: the description of a `CFF2` face (vg_manager_charstring2_font_desc) against
fontTools' view of the same table and against the reader's blend factors, its refusals, and the kit's strict interpreter
(tests/charstring2_edge_programs.py) run over the description against the host reader's command table — kinds as bytes,
coordinates as bits.  No device is needed."""
import io

import numpy as np
import pytest

from conftest import FIRA

pytest.importorskip("fontTools")
from fontTools.ttLib import TTFont  # noqa: E402

import charstring2_edge_programs as K2  # noqa: E402
from charstring_edge_programs import glyph_commands  # noqa: E402
from fira_cff_kit import fira_as_cff  # noqa: E402
from test_cff2_outlines import (_GLOBAL, _LOCAL, _NAMES, _PROGS, REGIONS, _build2, _variable_fira)  # noqa: E402


@pytest.fixture(scope="module")
def ops_cff2():
    return _build2(_NAMES, _PROGS, local_subrs=_LOCAL, global_subrs=_GLOBAL, extra_vardata=[(3, 0)])


@pytest.fixture(scope="module")
def fira_cff2():
    return _variable_fira()


def _desc(vg, font_bytes):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Face", font_bytes)
    return mgr, fid, mgr.charstring2_font_desc(fid, 0)


def assert_desc_invariants(d, n_glyph_ids):
    """what vgsdf_font_create_charstrings2 validates"""
    n_bytes = len(d["bytes"])
    assert n_bytes % 4 == 0 and len(d["cs_off"]) == n_glyph_ids + 1
    for k in ("cs_off", "gsubr_off", "lsubr_off"):
        o = d[k].astype(np.int64)
        assert len(o) >= 1 and (np.diff(o) >= 0).all() and o[-1] <= n_bytes, k
    assert d["fd_of"] is None and list(d["lsubr_first"]) == [0, len(d["lsubr_off"]) - 1]
    assert len(d["gsubr_off"]) - 1 <= 0xFFFF and len(d["lsubr_off"]) - 1 <= 0xFFFF
    so = d["set_off"].astype(np.int64)
    assert len(so) == len(d["set_ok"]) + 1 and so[0] == 0 and so[-1] == len(d["factors"])
    assert (np.diff(so) >= 0).all() and (np.diff(so) <= 64).all() and np.isfinite(d["factors"]).all()


def assert_equals_fonttools(d, font_bytes):
    """charstring, global and local subroutine bodies, and the region count of every set"""
    cff = TTFont(io.BytesIO(font_bytes))["CFF2"].cff
    top = cff.topDictIndex[0]
    blob = d["bytes"].tobytes()
    body = lambda off, i: blob[off[i]:off[i + 1]]   # noqa: E731
    index = top.CharStrings.charStringsIndex
    assert len(d["cs_off"]) - 1 == len(index)
    for g in range(len(index)):
        assert body(d["cs_off"], g) == index[g].bytecode, g
    assert len(d["gsubr_off"]) - 1 == len(cff.GlobalSubrs)
    for i in range(len(cff.GlobalSubrs)):
        assert body(d["gsubr_off"], i) == cff.GlobalSubrs[i].bytecode, i
    # the set the reader uses for every glyph: the first Font DICT that has local subroutines
    chosen = next((fd.Private.Subrs for fd in top.FDArray if getattr(fd.Private, "Subrs", None)), [])
    assert len(d["lsubr_off"]) - 1 == len(chosen)
    for i in range(len(chosen)):
        assert body(d["lsubr_off"], i) == chosen[i].bytecode, i
    store = top.VarStore.otVarStore
    assert len(d["set_ok"]) == len(store.VarData)
    for s, data in enumerate(store.VarData):
        assert d["set_ok"][s] == 1 and d["set_off"][s + 1] - d["set_off"][s] == len(data.VarRegionIndex), s


def _same_commands(host, kit):
    assert np.array_equal(host["cmd_off"], kit["cmd_off"]) and np.array_equal(host["dat_off"], kit["dat_off"])
    for g in range(len(host["cmd_off"]) - 1):
        assert glyph_commands(host, g) == glyph_commands(kit, g), g


def test_description_of_the_hand_written_blend_programs(vg, ops_cff2):
    mgr, fid, d = _desc(vg, ops_cff2)
    assert_desc_invariants(d, len(_NAMES))
    assert_equals_fonttools(d, ops_cff2)
    # the reader's factors at the default position: REGIONS peaks off 0 on some axis (0, 0, 0) or names no axis (1); the
    # second ItemVariationData holds regions 3 and 0
    assert len(REGIONS) == 4 and list(d["set_off"]) == [0, 4, 6] and list(d["factors"]) == [0, 0, 0, 1, 1, 0]
    again = mgr.charstring2_font_desc(fid, 0)                       # built once: the same table
    assert all(np.array_equal(d[k], again[k]) for k in d if d[k] is not None)
    kit, ends = K2.expected_commands(d, budget=1 << 62)
    assert ends == ["end"] * len(_NAMES)
    _same_commands(mgr.command_font_desc(fid, 0), kit)


def test_description_of_the_variable_fira_face(vg, fira_cff2):
    mgr, fid, d = _desc(vg, fira_cff2)
    assert_desc_invariants(d, TTFont(io.BytesIO(fira_cff2))["maxp"].numGlyphs)
    assert_equals_fonttools(d, fira_cff2)
    assert len(d["factors"]) >= 1 and not d["factors"].any()        # one axis, every region peaks at its maximum: 0 at the default
    host = mgr.command_font_desc(fid, 0)
    kit, ends = K2.expected_commands(d, budget=1 << 62)
    assert set(ends) == {"end"} and len(kit["kinds"]) > 5000
    _same_commands(host, kit)
    # the same table without `fvar`: the reader evaluates every region over no coordinates, every factor is 1
    f = TTFont(io.BytesIO(fira_cff2))
    for tag in ("fvar", "HVAR", "STAT"):
        if tag in f:
            del f[tag]
    buf = io.BytesIO()
    f.save(buf)
    mgr, fid, bare = _desc(vg, buf.getvalue())
    assert len(bare["factors"]) == len(d["factors"]) and (bare["factors"] == 1).all()
    host_bare = mgr.command_font_desc(fid, 0)
    assert host_bare["coords"].tobytes() != host["coords"].tobytes()
    _same_commands(host_bare, K2.expected_commands(bare, budget=1 << 62)[0])
    # (those factors as an argument over the first description: the interpreter's sets are data)
    _same_commands(host_bare, K2.expected_commands(d, sets=K2.blend_sets(bare), budget=1 << 62)[0])


@pytest.mark.parametrize("face", [K2.shared_face(), K2.set0_unusable_face(), K2.no_sets_face(), K2.sized_face(65)], ids=lambda f: f.name)
def test_description_and_interpreter_on_the_kit_faces(vg, face):
    """the kit's tables, written byte by byte: the host's description is the one the kit builds directly, and the interpreter
    delivers what the host reader delivers for every program"""
    mgr, fid, d = _desc(vg, face.font())
    assert_desc_invariants(d, len(face.glyphs))
    want = face.desc()
    for k, v in want.items():
        assert (d[k] is None) if v is None else np.array_equal(d[k], v), k
    kit, ends = K2.expected_commands(d, budget=1 << 62)
    _same_commands(mgr.command_font_desc(fid, 0), kit)
    by_name = dict(zip([n for n, _ in face.glyphs], ends))
    if face.name == "shared2":
        assert len(face.glyphs) > 150
        for name, end in (("stack_513", "end"), ("stack_514", "fail"), ("blend_one_short", "fail"), ("blend_exactly_the_stack", "end"),
                          ("blend_negative", "fail"), ("blend_fraction", "end"), ("blend_count_past_65535", "fail"), ("blend_empty_stack", "fail"),
                          ("blend_depth_10", "end"), ("depth_11", "fail"), ("vsindex_k2", "end"), ("vsindex_after_blend", "fail"),
                          ("vsindex_twice", "fail"), ("vsindex_2_operands", "fail"), ("vsindex_past_count", "fail"), ("vsindex_unusable", "fail"),
                          ("vsindex_too_many_regions", "fail"), ("return_mid_glyph", "fail"), ("endchar_mid_glyph", "fail"),
                          ("mask_past_end", "end"), ("mask_past_end_in_subr", "end"), ("ends_open", "end")):
            assert by_name[name] == end, name
        assert list(d["set_ok"]) == [1, 1, 1, 1, 1, 0, 0]
    if face.name in ("set0_unusable", "no_sets"):
        assert len(kit["kinds"]) == 0 and "end" not in ends           # without set 0 no glyph delivers anything
    # factors no default position produces change what blends deliver, and only that
    alt, alt_ends = K2.expected_commands(d, sets=K2.alt_sets(d), budget=1 << 62)
    if face.name == "shared2":
        assert alt["coords"].tobytes() != kit["coords"].tobytes()
        same = [n for n in by_name if not n.startswith(("blend", "vsindex", "depth"))]
        g_of = {n: g for g, (n, _) in enumerate(face.glyphs)}
        assert len(same) > 80 and all(glyph_commands(alt, g_of[n]) == glyph_commands(kit, g_of[n]) for n in same)


def test_budget_faces_are_what_the_kit_says(vg):
    at, over = K2.budget_faces()
    o = K2.interpret(at.desc(), 1)
    assert (o.end, o.tokens) == ("end", K2.MAX_TOKENS)
    mgr, fid, hd = _desc(vg, at.font())
    d = at.desc()
    assert all(np.array_equal(hd[k], d[k]) for k in d if d[k] is not None)
    assert glyph_commands(mgr.command_font_desc(fid, 0), 1)[0] == bytes(o.kinds) == bytes([K2.M, K2.L, K2.L])
    o = K2.interpret(over.desc(), 2)
    assert (o.end, o.tokens) == ("budget", K2.MAX_TOKENS + 1) and over.refusal == "budget"


def test_faces_without_a_description(vg):
    mgr = vg.FontManager(False)
    glyf = mgr.add_font_with_name("Fira", [FIRA])
    cff = mgr.add_font_data("CFF", fira_as_cff(40))
    for fid in (glyf, cff):
        with pytest.raises(RuntimeError, match="CFF2"):
            mgr.charstring2_font_desc(fid, 0)
    mgr.charstring_font_desc(cff, 0)                                  # (version 1 keeps its own description)
    cff2 = mgr.add_font_data("CFF2", K2.sized_face(3).font())
    mgr.charstring2_font_desc(cff2, 0)
    with pytest.raises(RuntimeError, match="CFF"):
        mgr.charstring_font_desc(cff2, 0)                             # ... and does not take a CFF2 face
    with pytest.raises(RuntimeError):
        mgr.charstring2_font_desc("nobody", 0)
    with pytest.raises(RuntimeError):
        mgr.charstring2_font_desc(cff2, 7)


def test_a_set_of_more_than_65535_subroutines_has_no_description(vg):
    """INDEX counts are 32 bits in CFF2; the device's description states at most 65535 subroutines per set"""
    glyphs = [(".notdef", K2.NOTDEF), ("line", K2.START + K2.enc(7, "hlineto"))]
    for n, described in ((65535, True), (65536, False)):
        for where in ("local", "global"):
            subrs = [b""] * n
            face = K2.Face(f"{where}_{n}", glyphs, subrs if where == "global" else [], subrs if where == "local" else [])
            mgr = vg.FontManager(False)
            fid = mgr.add_font_data("Face", face.font())
            if described:
                d = mgr.charstring2_font_desc(fid, 0)
                assert len(d["gsubr_off" if where == "global" else "lsubr_off"]) - 1 == n
            else:
                with pytest.raises(RuntimeError, match="CFF2"):
                    mgr.charstring2_font_desc(fid, 0)
            assert len(mgr.command_font_desc(fid, 0)["kinds"]) == 3   # (the host's way is there for all of them)
