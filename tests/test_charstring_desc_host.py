"""The host half of charstrings on the device: the description of a `CFF ` face (vg_manager_charstring_font_desc) against
fontTools' view of the same font, its refusals, and the kit's interpreter (tests/charstring_edge_programs.py) against the host
reader on every program — in callbacks as bits.  No device is needed."""
import io

import numpy as np
import pytest

from conftest import FIRA

pytest.importorskip("fontTools")
from fontTools.ttLib import TTFont  # noqa: E402

import charstring_edge_programs as K  # noqa: E402
from test_cff_outlines import fira_cff, ops_cff  # noqa: E402,F401  (fixtures)
from test_resident_commands_host import _cff2, _damage, fira_as_cff  # noqa: E402,F401


def _desc(vg, font_bytes):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Face", font_bytes)
    return mgr, fid, mgr.charstring_font_desc(fid, 0)


def assert_desc_invariants(d, n_glyph_ids):
    """what vgsdf_font_create_charstrings validates"""
    n_bytes = len(d["bytes"])
    assert n_bytes % 4 == 0 and len(d["cs_off"]) == n_glyph_ids + 1
    for k in ("cs_off", "gsubr_off", "lsubr_off"):
        o = d[k].astype(np.int64)
        assert len(o) >= 1 and (np.diff(o) >= 0).all() and o[-1] <= n_bytes, k
    first = d["lsubr_first"].astype(np.int64)
    assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] == len(d["lsubr_off"]) - 1 and 1 <= len(first) - 1 <= 256
    if d["fd_of"] is None:
        assert len(first) == 2
    else:
        assert len(d["fd_of"]) == n_glyph_ids and int(d["fd_of"].max()) < len(first) - 1


def assert_equals_fonttools(d, font_bytes):
    top = TTFont(io.BytesIO(font_bytes))["CFF "].cff.topDictIndex[0]
    cff = TTFont(io.BytesIO(font_bytes))["CFF "].cff
    blob = d["bytes"].tobytes()
    body = lambda off, i: blob[off[i]:off[i + 1]]   # noqa: E731
    index = top.CharStrings.charStringsIndex
    n = len(d["cs_off"]) - 1
    assert n == len(index)
    for g in range(n):
        assert body(d["cs_off"], g) == index[g].bytecode, g
    assert len(d["gsubr_off"]) - 1 == len(cff.GlobalSubrs)
    for i in range(len(cff.GlobalSubrs)):
        assert body(d["gsubr_off"], i) == cff.GlobalSubrs[i].bytecode, i
    privates = [fd.Private for fd in top.FDArray] if hasattr(top, "ROS") else [top.Private]
    first = d["lsubr_first"]
    assert len(first) - 1 == len(privates)
    for k, priv in enumerate(privates):
        subrs = getattr(priv, "Subrs", [])
        assert first[k + 1] - first[k] == len(subrs), k
        for i in range(len(subrs)):
            assert body(d["lsubr_off"], first[k] + i) == subrs[i].bytecode, (k, i)
    if hasattr(top, "ROS") and len(privates) > 1:
        assert [int(v) for v in d["fd_of"]] == [top.FDSelect[g] for g in range(n)]
    else:
        assert d["fd_of"] is None


def _small_face(cid):
    glyphs = [(".notdef", K.NOTDEF)] + [(f"g{i}", K.START + K.enc(i - 107, "callsubr", i, "hlineto", -107, "callgsubr", "endchar")) for i in range(1, 6)]
    sets = [[K.enc(i, i, "rlineto", "return") for i in range(1, 4)], [K.enc(9, "hlineto", "return")] * 2, []]
    gsubrs = [K.enc(-5, 40, "rlineto", "return"), K.RET]
    return K.Face("small", glyphs, gsubrs, sets if cid else sets[:1], [0, 0, 1, 2, 1, 0] if cid else None)


@pytest.mark.parametrize("off_size", [1, 2, 3, 4])
@pytest.mark.parametrize("cid", [False, True], ids=["name_keyed", "cid_keyed"])
def test_description_equals_fonttools_for_every_index_offsize(vg, cid, off_size):
    face = _small_face(cid)
    font = face.font(off_size)
    cff = TTFont(io.BytesIO(font))["CFF "].cff
    assert cff.topDictIndex[0].CharStrings.charStringsIndex is not None
    _, _, d = _desc(vg, font)
    assert_desc_invariants(d, len(face.glyphs))
    assert_equals_fonttools(d, font)
    want = face.desc()
    for k, v in want.items():
        assert (d[k] is None) if v is None else np.array_equal(d[k], v), k


def test_description_of_the_fonttools_built_fonts(vg, fira_cff, ops_cff):  # noqa: F811
    for font in (fira_cff, ops_cff):
        mgr, fid, d = _desc(vg, font)
        assert_desc_invariants(d, TTFont(io.BytesIO(font))["maxp"].numGlyphs)
        assert_equals_fonttools(d, font)
        again = mgr.charstring_font_desc(fid, 0)                   # built once: the same table
        assert all(np.array_equal(d[k], again[k]) for k in d if d[k] is not None)


@pytest.mark.parametrize("face", [K.shared_face(), K.cid_face()] + K.bias_faces(), ids=lambda f: f.name)
def test_description_of_the_kit_faces(vg, face):
    font = face.font()
    _, _, d = _desc(vg, font)
    assert_desc_invariants(d, len(face.glyphs))
    assert_equals_fonttools(d, font)


def test_faces_without_a_description(vg):
    mgr = vg.FontManager(False)
    glyf = mgr.add_font_with_name("Fira", [FIRA])
    with pytest.raises(RuntimeError, match="CFF"):
        mgr.charstring_font_desc(glyf, 0)
    cff2 = mgr.add_font_data("CFF2", _cff2())
    with pytest.raises(RuntimeError, match="CFF"):
        mgr.charstring_font_desc(cff2, 0)
    with pytest.raises(RuntimeError):
        mgr.charstring_font_desc("nobody", 0)
    with pytest.raises(RuntimeError):
        mgr.charstring_font_desc(glyf, 7)
    mgr.command_font_desc(glyf, 0)                                  # (the command table is there for all of them)
    mgr.command_font_desc(cff2, 0)


def _same_commands(host, kit, skip=()):
    assert np.array_equal(host["cmd_off"], kit["cmd_off"]) or skip
    for g in range(len(host["cmd_off"]) - 1):
        if g not in skip:
            assert K.glyph_commands(host, g) == K.glyph_commands(kit, g), g


@pytest.mark.parametrize("seed", [1, 2])
def test_damaged_cff_tables_are_refused_or_described_soundly(vg, fira_as_cff, seed):  # noqa: F811
    """the damage of tests/test_resident_commands_host.py: a mutant that loads has no description (-1) or one that holds what
    the device will be promised; the first described mutants are also interpreted from their description, against the reader"""
    rng = np.random.default_rng(seed)
    n_refused = n_described = n_interpreted = 0
    for i in range(1, 40):
        mutant = _damage(fira_as_cff, rng, i)
        mgr = vg.FontManager(False)
        try:
            fid = mgr.add_font_data(f"Mutant {i}", mutant)
        except RuntimeError:
            continue
        try:
            d = mgr.charstring_font_desc(fid, 0)
        except RuntimeError:
            n_refused += 1
            continue
        n_described += 1
        host = mgr.command_font_desc(fid, 0)
        assert_desc_invariants(d, len(host["cmd_off"]) - 1)
        if n_interpreted < 3:
            n_interpreted += 1
            kit, ends = K.expected_commands(d)
            _same_commands(host, kit, skip={g for g, e in enumerate(ends) if e == "seac"})
    print(f"seed {seed}: {n_described} mutants described, {n_refused} refused")
    assert n_described >= 1


def _kit_against_reader(vg, face):
    mgr, fid, d = _desc(vg, face.font())
    host = mgr.command_font_desc(fid, 0)
    kit, ends = K.expected_commands(d, budget=1 << 62)           # (the host reader has no budget)
    seac = {g for g, e in enumerate(ends) if e == "seac"}
    _same_commands(host, kit, skip=seac)
    return ends, seac


def test_the_kits_interpreter_agrees_with_the_host_reader_on_every_program(vg):
    face = K.shared_face()
    ends, seac = _kit_against_reader(vg, face)
    by_name = {name: ends[g] for g, (name, _) in enumerate(face.glyphs)}
    assert not seac and len(face.glyphs) > 140
    # the end states the programs were written for
    for name, want in (("numbers", "endchar"), ("cut_247", "fail"), ("cut_255_3", "fail"), ("stack_48", "endchar"), ("stack_49", "fail"),
                       ("depth_10", "endchar"), ("depth_11", "fail"), ("subr_below_0", "fail"), ("subr_past_count", "fail"),
                       ("mask_0_stems", "endchar"), ("mask_8_stems", "endchar"), ("mask_9_stems", "endchar"), ("mask_past_end", "fail"),
                       ("mask_implied_vstem", "endchar"), ("width_twice_hmoveto", "fail"), ("width_twice_endchar", "endchar"),
                       ("no_move_rlineto", "fail"), ("flex1_equal", "endchar"), ("flex_12", "fail"), ("escape_unsupported", "fail"),
                       ("reserved_2", "fail"), ("endchar_in_subr", "endchar"), ("endchar_in_subr_data_behind_call", "fail"),
                       ("data_after_endchar", "fail"), ("no_endchar", "end"), ("return_at_top", "return"), ("empty", "end")):
        assert by_name[name] == want, name
    # the same programs in another order, as one face each (a sample), and the faces with their own subroutine sets
    rng = np.random.default_rng(5)
    _kit_against_reader(vg, K.shared_face(order=rng.permutation(len(face.glyphs) - 1), name="shuffled"))
    for single in K.single_faces()[::9]:
        _kit_against_reader(vg, single)
    for other in K.bias_faces() + [K.cid_face(), K.long_face(), K.sized_face(129, empty={0, 128} | set(range(1, 128, 2)))]:
        ends, seac = _kit_against_reader(vg, other)
        assert not seac and "fail" in ends or other.name.startswith(("long", "sized"))


def test_bias_steps_and_font_dicts_select_other_subroutines(vg):
    by = {}
    for face in K.bias_faces():
        _, _, d = _desc(vg, face.font())
        by[face.name] = dict(zip([n for n, _ in face.glyphs], K.expected_commands(d)[1]))
    assert by["local_1239"]["last"] == by["local_1240"]["last"] == "endchar"
    assert by["local_1239"]["past_count"] == by["local_1240"]["past_count"] == "fail"
    assert by["local_1239"]["below_0"] == by["local_1240"]["below_0"] == by["global_33899"]["below_0"] == "fail"
    assert by["global_33899"]["last"] == by["global_33900"]["last"] == by["global_33900"]["first"] == "endchar"
    assert by["global_33900"]["past_count"] == "fail"
    cid = K.cid_face()
    ends = K.expected_commands(cid.desc())[1]
    by_name = dict(zip([n for n, _ in cid.glyphs], ends))
    assert (by_name["op-104_fd0"], by_name["op-104_fd1"], by_name["op-104_fd2"]) == ("endchar", "endchar", "fail")   # 3 of 1239, 1027 of 1240, 3 of 3
    assert (by_name["op-1131_fd0"], by_name["op-1131_fd1"], by_name["op-1131_fd2"]) == ("fail", "endchar", "fail")
    assert (by_name["op1132_fd0"], by_name["op1132_fd1"]) == ("fail", "fail")                                          # 1239 of 1239, 2263 of 1240
    assert (by_name["op108_fd0"], by_name["op108_fd1"], by_name["op108_fd2"]) == ("endchar", "endchar", "fail")


def test_seac_and_budget_are_what_the_kit_says(vg):
    for face in K.seac_faces():
        ends, seac = _kit_against_reader(vg, face)
        assert seac == {2} and face.refusal == "seac"
    at, over = K.budget_faces()
    d = at.desc()
    o = K.interpret(d, 1)
    assert (o.end, o.tokens) == ("endchar", K.MAX_TOKENS)
    mgr, fid, hd = _desc(vg, at.font())
    assert all(np.array_equal(hd[k], d[k]) for k in d if d[k] is not None)
    host = mgr.command_font_desc(fid, 0)
    assert K.glyph_commands(host, 1)[0] == bytes(o.kinds)
    o = K.interpret(over.desc(), 2)
    assert (o.end, o.tokens) == ("budget", K.MAX_TOKENS + 1) and over.refusal == "budget"
