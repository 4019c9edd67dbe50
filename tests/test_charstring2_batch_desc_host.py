"""The host half of "all instances of a CFF2 file in one device build", no device needed.

The batched description (vg_manager_charstring2_fonts_desc) of the instance group a named-instance file makes: position p's slice
of the factors is vg_manager_charstring2_font_desc of instance p, every other array is instance 0's (and, one file having one
parse, every instance's); the cases without a description.

The kit's position-dependent programs (tests/charstring2_batch_kit.py): at the chosen positions the glyphs' command counts really
differ — by the strict interpreter AND by the host reader, whose callbacks are compared with the interpreter's, kinds as bytes,
coordinates as bits.  Without that the GPU test of these programs (tests/test_gpu_charstring2_batch_regimes.py) would prove
nothing."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring2_batch_kit as B  # noqa: E402
import named_instances_kit as N  # noqa: E402
import variable_instances_kit as V  # noqa: E402
from charstring_edge_programs import glyph_commands  # noqa: E402
from conftest import FIRA  # noqa: E402

ARRAYS = ("bytes", "cs_off", "gsubr_off", "lsubr_first", "lsubr_off", "set_ok", "set_off")


@pytest.mark.parametrize("which", ["one_axis", "two_axes", "merged_ids"])
def test_the_batched_description_is_the_single_ones_side_by_side(vg, which):
    font, records = B.instance_files()[which]
    mgr = vg.FontManager(False)
    ids = mgr.add_font_named_instances(font)
    assert ids == N.instance_ids(vg, font) and len(ids) == len(records)
    own = [i for i in ids if ids.count(i) == 1]
    assert len(own) == {"one_axis": 9, "two_axes": 3, "merged_ids": 2}[which]
    group = mgr.instance_group(own[0])
    assert group == ids
    # the faces of the group, in its order: a merged id holds two of them, file 0 and file 1
    seen, singles = {}, []
    for i in group:
        singles.append(mgr.charstring2_font_desc(i, seen.get(i, 0)))
        seen[i] = seen.get(i, 0) + 1
    for fid in own:                                                     # whichever id of the group is asked
        d = mgr.charstring2_fonts_desc(fid)
        assert d["fd_of"] is None and d["positions"].shape == (len(group), len(singles[0]["factors"]))
        for k in ARRAYS:
            assert np.array_equal(d[k], singles[0][k]), k
        for p, single in enumerate(singles):
            assert d["positions"][p].tobytes() == single["factors"].tobytes(), p
            for k in ARRAYS:
                assert np.array_equal(single[k], singles[0][k]), (p, k)
    # the positions are positions: the factors differ between the records, and follow the axes
    d = mgr.charstring2_fonts_desc(own[0])
    assert len({d["positions"][p].tobytes() for p in range(len(group))}) >= 3
    assert len(d["factors"]) >= (2 if which == "two_axes" else 1) and np.isfinite(d["positions"]).all()


def test_font_ids_without_a_batched_description(vg):
    font, records = B.instance_files()["merged_ids"]
    mgr = vg.FontManager(False)
    ids = mgr.add_font_named_instances(font)
    merged = [i for i in set(ids) if ids.count(i) == 2]
    assert len(merged) == 2
    for fid in merged:
        with pytest.raises(RuntimeError, match="group"):
            mgr.charstring2_fonts_desc(fid)                             # an id of two files
    with pytest.raises(RuntimeError):
        mgr.charstring2_fonts_desc("nobody")
    # a file placed alone keeps its own copy: in no group
    alone = mgr.add_font_instance("Alone", font, {"wght": 650})
    mgr.charstring2_font_desc(alone, 0)
    with pytest.raises(RuntimeError, match="group"):
        mgr.charstring2_fonts_desc(alone)
    # a static CFF2 file, a glyf file, the named instances of a glyf file: where the single description says no, and in no group
    plain = mgr.add_font_data("Plain", V.variable_fira(40))
    with pytest.raises(RuntimeError, match="group"):
        mgr.charstring2_fonts_desc(plain)
    glyf = mgr.add_font_with_name("Fira", [FIRA])
    with pytest.raises(RuntimeError, match="CFF2"):
        mgr.charstring2_fonts_desc(glyf)
    gvar_font, _ = N.files()["two_axes_no_room"]
    for fid in set(mgr.add_font_named_instances(gvar_font)):
        with pytest.raises(RuntimeError, match="CFF2"):
            mgr.charstring2_fonts_desc(fid)


def _host_and_interpreter_at(vg, face, wght):
    """(the face's description with the host reader's factors at `wght`, the interpreter's commands under them, its ends), the
    host reader's commands held against the interpreter's as bits"""
    mgr = vg.FontManager(False)
    fid = mgr.add_font_instance("At", face.font(), {"wght": wght})
    d, host = mgr.charstring2_font_desc(fid, 0), mgr.command_font_desc(fid, 0)
    want = face.desc()
    for k in ARRAYS:
        assert np.array_equal(d[k], want[k]), k
    kit, ends = B.expected_commands(d, budget=1 << 62)
    assert np.array_equal(host["cmd_off"], kit["cmd_off"]) and np.array_equal(host["dat_off"], kit["dat_off"])
    for g in range(len(face.glyphs)):
        assert glyph_commands(host, g) == glyph_commands(kit, g), g
    return d, kit, ends


def test_the_position_dependent_programs_deliver_different_counts_at_different_positions(vg):
    face = B.position_dependent_face()
    g_of = {n: g for g, (n, _) in enumerate(face.glyphs)}
    counts, ends_at = {}, {}
    for f, wght in ((0.0, 400), (0.5, 650), (1.0, 900), (0.3, 550)):
        d, kit, ends = _host_and_interpreter_at(vg, face, wght)
        assert len(d["factors"]) == 1 and abs(float(d["factors"][0]) - f) < 1e-4 and (f == 0.3 or float(d["factors"][0]) == f)
        counts[f], ends_at[f] = np.diff(kit["cmd_off"].astype(np.int64)), ends
        # ... and the interpreter under the literal factor the GPU test sends says the same counts
        lit, lit_ends = B.expected_commands(dict(d, factors=np.array([f], np.float32)))
        assert np.array_equal(np.diff(lit["cmd_off"].astype(np.int64)), counts[f]) and lit_ends == ends
    for name in B.POSITION_DEPENDENT:
        g = g_of[name]
        for f, lines in B.LINES_AT[name].items():
            assert counts[f][g] == (1 if lines is None else 1 + lines), (name, f)
            assert ends_at[f][g] == ("fail" if lines is None else "end"), (name, f)
        assert len({int(counts[f][g]) for f in counts}) >= 2, name                 # the counts differ between positions
    # a blended index: a delta of 1 moves it by one subroutine; an integer at one position, none at another
    assert counts[0.0][g_of["blended_callsubr"]] != counts[1.0][g_of["blended_callsubr"]]
    assert ends_at[0.3][g_of["blended_callsubr"]] == "fail" and ends_at[1.0][g_of["blended_callsubr"]] == "end"
    assert ends_at[0.5][g_of["blended_callgsubr_by_halves"]] == "end" and ends_at[0.3][g_of["blended_callgsubr_by_halves"]] == "fail"
    # a blended blend count
    assert counts[0.0][g_of["blended_blend_count"]] == 4 and counts[1.0][g_of["blended_blend_count"]] == 3
    # the plain neighbours do not move
    for name in ("plain_a", "plain_b", "plain_c"):
        assert len({int(counts[f][g_of[name]]) for f in counts}) == 1 and all(ends_at[f][g_of[name]] == "end" for f in counts)


def test_the_budget_is_passed_at_one_position_only(vg):
    face = B.budget_by_position_face()
    d = face.desc()
    got = {f: B.interpret(dict(d, factors=np.array([f], np.float32)), 2) for f in (0.0, 1.0, 0.3)}
    assert (got[0.0].end, got[0.0].tokens) == ("end", B.MAX_TOKENS)
    assert (got[1.0].end, got[1.0].tokens) == ("budget", B.MAX_TOKENS + 1)
    assert (got[0.3].end, got[0.3].tokens, len(got[0.3].kinds)) == ("fail", 5, 0)
    # the host reader at the axis' ends: the same commands as the interpreter (it has no budget: the device's refusal is the
    # device's), and the host's description is the kit's
    for wght, f in ((400, 0.0), (900, 1.0)):
        hd, kit, ends = _host_and_interpreter_at(vg, face, wght)
        assert float(hd["factors"][0]) == f and ends == ["end"] * 3 and len(glyph_commands(kit, 2)[0]) == 3
