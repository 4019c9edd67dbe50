"""Rule G7 of csrc/host/ttf_face.hpp on the host: a placed `glyf` face without `HVAR` takes its advances from gvar's phantom
points when the manager's switch (set_gvar_advances) was on at placement, and keeps `hmtx` when it was off.

Checked against the strict restatement of tests/phantom_advances_kit.py bit for bit, and against fontTools' widths at the
positions whose scalars are dyadic (both round by floor(x + 0.5)).
"""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
import phantom_advances_kit as P  # noqa: E402
import variable_instances_kit as K  # noqa: E402

TWO_AXES = [{"wght": 650, "wdth": 100}, {"wght": 775, "wdth": 150}, {"wght": 900, "wdth": 200}]


def _placed(vg, font, on, location=None, coords=None, name="Inst", cpu=False):
    mgr = vg.FontManager(cpu)
    mgr.set_gvar_advances(on)
    fid = mgr.add_font_instance(name, font, location) if coords is None else mgr.add_font_instance_normalized(name, font, coords)
    return mgr, fid


def _all_faces():
    return [(case, font) for case, (font, _) in P.faces().items()] + [("truncated", P.truncated_face())]


def test_with_the_switch_off_the_hmtx_advance_stands_on_every_face(vg):
    for case, font in _all_faces():
        for position in ([16384], [5000]):
            mgr, fid = _placed(vg, font, False, coords=position)
            assert mgr.font_hor_advances(fid).tolist() == P.hmtx_advances(font).tolist(), case
            assert mgr.gvar_advance_stats() == {"faces": 0, "device_builds": 0, "fallbacks": 0}
    font = P.without_hvar("shear")
    mgr, fid = _placed(vg, font, False, {"wght": 650})
    assert mgr.font_hor_advances(fid).tolist() == P.hmtx_advances(font).tolist()


def test_advances_and_deltas_are_the_restatement_bit_for_bit_on_every_hand_written_face(vg):
    moved = 0
    for case, font in _all_faces():
        for position in P.POSITIONS:
            mgr, fid = _placed(vg, font, True, coords=position)
            assert mgr.gvar_advance_stats() == {"faces": 1, "device_builds": 0, "fallbacks": 0}
            want_d, want_state = P.restate_deltas(font, position)
            got_d, got_state = mgr.font_gvar_advance_deltas(fid)
            assert got_state.tolist() == want_state.tolist(), (case, position)
            assert G.bits(got_d) == G.bits(want_d), (case, position)
            want = P.restate_advances(font, position)
            assert mgr.font_hor_advances(fid).tolist() == want.tolist(), (case, position)
            moved += int((want != P.hmtx_advances(font)).sum())
    assert moved > 100


def test_the_hand_written_faces_hold_what_they_are_there_for(vg):
    faces = P.faces()
    at = lambda case, position=(16384,): P.restate_deltas(faces[case][0], list(position))  # noqa: E731
    d, state = at("empty_entries")
    assert d.tolist() == [14.0, 40.0, 33.0, 9.0, 0.0] and state.tolist() == [1, 1, 1, 1, 0]
    d, state = at("point_lists")
    assert d.tolist()[:8] == [14.0, -40.0, -25.0, 59.0, 0.0, 28.0, 16.0, 77.0] and d[8] == 10.0 and set(state.tolist()) == {1}
    d, _ = at("delta_runs")
    assert len(set(d.tolist()[1:10])) >= 5 and d[10] != 0 and d[11] != 0   # zero, byte and word runs read different values
    d, state = at("scalars", (5000,))
    assert state.tolist() == [1, 1, 1, 1] and d[1] != 0 and d[2] != 0
    # the order of the f32 sums matters for the two tuples that both move r: another order gives another value somewhere
    s = [P.f32(5000) / P.f32(16384), P.f32(5000) / P.f32(8192)]
    in_order = P.f32(P.f32(P.f32(P.f32(333) * s[0]) + P.f32(P.f32(-77) * s[1])) + P.f32(P.f32(1001) * s[0]))
    assert d[2] == in_order
    d, state = at("composites")
    assert d.tolist() == [14.0, 200.0, 1.0, 80.0, -3.0, 21.0, 0.0] and state.tolist() == [1, 1, 1, 1, 1, 1, 0]
    d, state = at("malformed")
    assert {g for g, s in enumerate(state.tolist()) if s == P.MALFORMED} == faces["malformed"][1] == {1, 2, 3, 4}
    adv = P.restate_advances(faces["out_of_range"][0], [16384]).tolist()
    assert adv[1:] == [0, 0, 0, 0, 65535, 0]
    # every truncation of a glyph's data but the whole of it (and none of it) is malformed where its tuples apply
    _, state = P.restate_deltas(P.truncated_face(), [8192])
    assert state[0] == P.NONE and state[-1] == P.DELTA and all(s == P.MALFORMED for s in state[1:-1])


def test_malformed_ids_keep_hmtx(vg):
    font, malformed = P.faces()["malformed"]
    mgr, fid = _placed(vg, font, True, coords=[16384])
    got, hmtx = mgr.font_hor_advances(fid).tolist(), P.hmtx_advances(font).tolist()
    for g in malformed:
        assert got[g] == hmtx[g]
    assert got[0] != hmtx[0] and got[5] != hmtx[5]
    font = P.truncated_face()
    mgr, fid = _placed(vg, font, True, coords=[8192])
    got, hmtx = mgr.font_hor_advances(fid).tolist(), P.hmtx_advances(font).tolist()
    assert got[:-1] == hmtx[:-1] and got[-1] != hmtx[-1]
    # ids past numGlyphs have no advance
    assert mgr.font_hor_advances(fid, extra=3).tolist()[-3:] == [0, 0, 0]


@pytest.mark.parametrize("kind, locations", [("shear", G.EXACT_ONE_AXIS), ("scale", G.EXACT_ONE_AXIS), ("two_axes", G.EXACT_ONE_AXIS + TWO_AXES)])
def test_the_fixtures_without_hvar_equal_the_restatement_and_fonttools(vg, kind, locations):
    font = P.without_hvar(kind)
    hmtx = P.hmtx_advances(font)
    for loc in locations:
        mgr, fid = _placed(vg, font, True, loc)
        coords = mgr.font_position(fid)
        assert coords == K.coords_of(font, loc)
        got = mgr.font_hor_advances(fid)
        assert got.tolist() == P.restate_advances(font, coords).tolist(), loc
        d, state = mgr.font_gvar_advance_deltas(fid)
        want_d, want_state = P.restate_deltas(font, coords)
        assert G.bits(d) == G.bits(want_d) and state.tolist() == want_state.tolist()
        if "wdth" not in loc:                                  # the positions whose scalars are dyadic
            assert got.tolist() == P.fonttools_advances(font, loc), loc
            if loc == {"wght": 650}:
                assert len(got) == 315 and int((got != hmtx).sum()) == 315
        assert int((got != hmtx).sum()) > 250


def test_files_that_keep_their_hvar_are_unchanged_by_the_switch(vg):
    for kind, loc in (("shear", {"wght": 650}), ("two_axes", {"wght": 775, "wdth": 150})):
        font = G.variable_glyf_fira(kind)
        off, fo = _placed(vg, font, False, loc)
        on, fn = _placed(vg, font, True, loc)
        assert on.gvar_advance_stats() == {"faces": 0, "device_builds": 0, "fallbacks": 0}
        assert on.font_hor_advances(fn).tolist() == off.font_hor_advances(fo).tolist()
        G.same_family(on.family_desc(fn), off.family_desc(fo))
        a, b = on.record_outlines(fn), off.record_outlines(fo)
        for k in ("cmd_off", "cmds", "scale", "shift_x", "ids", "advances"):
            assert G.bits(a[k]) == G.bits(b[k]), k


def test_the_switch_is_not_retroactive_and_static_faces_do_not_see_it(vg):
    font = P.without_hvar("shear")
    mgr = vg.FontManager(False)
    before = mgr.add_font_instance("Before", font, {"wght": 650})
    mgr.set_gvar_advances(True)
    after = mgr.add_font_instance("After", font, {"wght": 650})
    plain = mgr.add_font_data("Plain", font)
    hmtx = P.hmtx_advances(font).tolist()
    assert mgr.font_hor_advances(before).tolist() == hmtx == mgr.font_hor_advances(plain).tolist()
    assert mgr.font_hor_advances(after).tolist() != hmtx
    assert mgr.gvar_advance_stats() == {"faces": 1, "device_builds": 0, "fallbacks": 0}


def test_families_outlines_and_named_instances_follow(vg):
    import named_instances_kit as N
    font = P.without_hvar("shear")
    mgr, fid = _placed(vg, font, True, {"wght": 650})
    coords = mgr.font_position(fid)
    want = P.restate_advances(font, coords)
    fam = mgr.family_desc(fid)
    assert len(fam["glyph_id"]) > 250
    upem = 1000
    for gid, adv in zip(fam["glyph_id"].tolist(), fam["advance"].tolist()):
        assert adv == int(np.floor(float(want[gid]) * (24.0 / upem) * 0.95 + 0.5))
    off, fo = _placed(vg, font, False, {"wght": 650})
    assert G.bits(off.family_desc(fo)["advance"]) != G.bits(fam["advance"])
    assert G.bits(off.family_desc(fo)["shift_x"]) != G.bits(fam["shift_x"])
    # the outlines themselves do not move: the left phantom point shifts nothing
    a, b = mgr.command_font_desc(fid), off.command_font_desc(fo)
    assert G.bits(a["coords"]) == G.bits(b["coords"])
    # named instances: every instance record placed with the switch on follows
    named = N.with_instances(font, N.ONE_AXIS)
    m = vg.FontManager(False)
    m.set_gvar_advances(True)
    ids = m.add_font_named_instances(named)
    assert len(ids) == len(N.ONE_AXIS) and m.gvar_advance_stats() == {"faces": len(ids), "device_builds": 0, "fallbacks": 0}
    met = {}
    for i, record in zip(ids, N.ONE_AXIS):
        k = met[i] = met.get(i, -1) + 1                                   # (two records may share a font id: its files, in order)
        assert m.font_position(i, k) == K.coords_of(font, record["location"])
        assert m.font_hor_advances(i, k).tolist() == P.restate_advances(named, m.font_position(i, k)).tolist()
    assert m.font_hor_advances(ids[1]).tolist() == want.tolist()          # the record at wght 650


def test_instance_to_pbf_with_the_dummy_raster_equals_the_yardstick(oracle, vg):
    """whole path on the CPU: the files of the instance at wght 650 = fontTools' points and phantom widths through the oracle"""
    font = P.without_hvar("shear")
    mgr, fid = _placed(vg, font, True, {"wght": 650}, name="Fira Medium", cpu=True)
    w = vg.DummyWriter()
    mgr.render_glyphs(w, vg.Renderer.new_dummy())
    want = P.yardstick_files(font, {"wght": 650}, fid, oracle, mode=oracle.DUMMY)
    assert len(want) == 256
    for path, data in want.items():
        assert w.files[path] == data, path
    off, fo = _placed(vg, font, False, {"wght": 650}, name="Fira Medium", cpu=True)
    w2 = vg.DummyWriter()
    off.render_glyphs(w2, vg.Renderer.new_dummy())
    assert fo == fid and sum(w2.files[p] != w.files[p] for p in want) >= 1
