"""A variable `glyf` file at a chosen position of its design space, on the host: the `gvar` reader (rules G1 to G6 of
csrc/host/ttf_face.hpp) and what the façade makes of such a face — a command face, never a glyf one.

The rules are written from the OpenType specification; the crate is not at hand, so PARITY WITH THE CRATE IS UNPINNED, as for the
rest of the variation code.  What is checked: the reader against fontTools' glyph set at a location (exactly where every value
is exact in f32, within a derived bound where points are inferred) and, bit for bit, against the strict restatement of
tests/gvar_instances_kit.py, on fonts built here and on hand-written tables at the edges of the rules.
"""
import io
import math

import numpy as np
import pytest

pytest.importorskip("fontTools")
from fontTools.ttLib import TTFont  # noqa: E402

import gvar_instances_kit as G  # noqa: E402
import variable_instances_kit as K  # noqa: E402

TABLE_KEYS = ("cmd_off", "dat_off", "kinds", "coords")


def _placed(vg, font, location=None, coords=None, name="Inst"):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_instance(name, font, location) if coords is None else mgr.add_font_instance_normalized(name, font, coords)
    return mgr, fid


def _edge_coords(case, position):
    return position if case != "two_axes" else [position[0], -position[0] // 2 if position[0] > 0 else 16384]


@pytest.mark.parametrize("kind, locations", [("shear", G.EXACT_ONE_AXIS), ("two_axes", G.EXACT_TWO_AXES)])
def test_outlines_and_advances_at_exact_positions_equal_fonttools(vg, kind, locations):
    font = G.variable_glyf_fira(kind)
    upem = TTFont(io.BytesIO(font), lazy=True)["head"].unitsPerEm
    default = G.fonttools_callbacks(font, {})[0]
    for loc in locations:
        want, widths, seen = G.fonttools_callbacks(font, loc)
        mgr, fid = _placed(vg, font, loc)
        o = mgr.record_outlines(fid)
        got = G.callbacks_of(o)
        assert set(got) == set(want) and len(got) > 250 and len(seen) > 19000
        for cp in want:
            assert got[cp] == want[cp], (loc, hex(cp))
        assert sum(want[cp] != default[cp] for cp in want) > 250
        for i, cp in enumerate(o["ids"]):
            w = widths[int(cp)]
            assert int(o["advances"][i]) == int(math.floor(math.floor(w + 0.5) * (24.0 / upem) * 0.95 + 0.5)), (loc, hex(int(cp)))
        G.same_family(mgr.family_desc(fid), K.family_entries([(font, K.coords_of(font, loc))]))
    # the fixture holds what it is there for: simple glyphs and composites, and (c) intermediate regions and shared tuples
    f = TTFont(io.BytesIO(font))
    assert sum(f["glyf"][g].isComposite() for g in f.getGlyphOrder()) >= 8 and len(f.getGlyphOrder()) == 315
    if kind == "two_axes":
        tuples = [t for g in f.getGlyphOrder() for t in f["gvar"].variations.get(g, [])]
        assert any(v[0] != min(v[1], 0) or v[2] != max(v[1], 0) for t in tuples for v in t.axes.values())
        assert int.from_bytes(K._table(font, "gvar")[6:8], "big") >= 2          # sharedTupleCount


@pytest.mark.parametrize("kind, locations", [("shear", G.EXACT_ONE_AXIS + [{"wght": 700}]), ("scale", G.EXACT_ONE_AXIS + [{"wght": 700}]),
                                             ("two_axes", G.EXACT_TWO_AXES + [{"wght": 700, "wdth": 130}])])
def test_the_reader_is_the_restatement_bit_for_bit_on_the_fixtures(vg, kind, locations):
    font = G.variable_glyf_fira(kind)
    for loc in locations:
        mgr, fid = _placed(vg, font, loc)
        coords = mgr.font_position(fid)
        assert coords == K.coords_of(font, loc)
        got, want = mgr.command_font_desc(fid), G.restate(font, coords)
        for key in TABLE_KEYS:
            assert G.bits(got[key]) == G.bits(want[key]), (loc, key)
        assert len(got["kinds"]) > 8000


def test_the_reader_is_the_restatement_bit_for_bit_on_every_hand_written_face(vg):
    n = 0
    for case, (font, malformed) in G.edge_faces().items():
        plain = vg.FontManager(False)
        static = plain.command_font_desc(plain.add_font_data("Edge", font))
        for position in G.EDGE_POSITIONS:
            coords = _edge_coords(case, position)
            mgr, fid = _placed(vg, font, coords=coords, name="Edge")
            got, want = mgr.command_font_desc(fid), G.restate(font, coords)
            for key in TABLE_KEYS:
                assert G.bits(got[key]) == G.bits(want[key]), (case, coords, key)
            n += 1
            if position == [16384]:
                # every glyph id's tuples apply there: the malformed ones are those the case names, they deliver nothing of
                # their own, and the face differs from the static one
                refused = {g for g, ok in enumerate(want["ok"]) if not ok}
                if malformed is not None:
                    assert refused == malformed, case
                assert G.bits(got["coords"]) != G.bits(static["coords"]), case
            # what a glyph id delivers does not depend on whether outline_glyph says false behind it: ids and advances stay
            o = mgr.record_outlines(fid)
            assert len(o["ids"]) == len(want["ok"])
    assert n == 5 * len(G.edge_faces()) >= 55
    # truncation at every byte: a glyph id with fewer bytes than its tuples need is malformed, the whole data is not
    font = G.edge_faces()["truncated"][0]
    ok = G.restate(font, [8192])["ok"]
    assert ok[0] and ok[-1] and sum(not v for v in ok) == len(ok) - 2
    # a malformed child: the leaves in front of it stay, nothing comes behind it
    font = G.edge_faces()["composites_malformed"][0]
    t = G.restate(font, [16384])
    assert t["cmd_off"][3] - t["cmd_off"][2] == 6 and t["cmd_off"][2] - t["cmd_off"][1] == 0 == t["cmd_off"][4] - t["cmd_off"][3]


def test_inferred_points_are_close_to_fonttools(vg):
    """(b): 298 of the 315 tuples leave points to inference and the values are not exact in f32.  Bound: a coordinate of the
    reader is f32(i16) + a, the sum of at most one tuple per axis region here (one tuple), whose inferred delta takes one
    product (the scaling of da and db each), one divide, one difference, two products and one sum, then the accumulator's sum
    and the point's sum: 8 roundings; the emitter adds 3 for an implied midpoint, a composite's transform 4 per coordinate and
    2 for its offset's own sums.  Every intermediate value is below 4096 in magnitude (asserted), so each rounding is at most
    half an ulp of that, 2^-13: 17 * 2^-13 font units.  fontTools works in f64 from the same normalised coordinate.  The deviation
    seen is 7.1e-5 font units."""
    font = G.variable_glyf_fira("scale")
    f = TTFont(io.BytesIO(font))
    inferred = sum(None in t.coordinates for g in f.getGlyphOrder() for t in f["gvar"].variations.get(g, []))
    assert inferred == 298, inferred
    bound, worst = 17 * 2.0 ** -13, 0.0
    for loc in G.EXACT_ONE_AXIS + [{"wght": 700}]:
        mgr, fid = _placed(vg, font, loc)
        coords = mgr.font_position(fid)
        want, _, seen = G.fonttools_callbacks(font, {"wght": coords[0] / 16384.0}, exact=False, normalized=True)
        assert max(abs(v) for v in seen) < 4096
        got = G.callbacks_of(mgr.record_outlines(fid))
        for cp in want:
            assert [t[0] for t in got[cp]] == [t[0] for t in want[cp]], hex(cp)
            for a, b in zip(got[cp], want[cp]):
                for u, v in zip(a[1:], b[1:]):
                    worst = max(worst, abs(u - v))
                    assert abs(u - v) <= bound and abs(v) < 4096, (loc, hex(cp), u, v)
    print(f"largest deviation from fontTools on the pure-scale fixture: {worst!r} font units (bound {bound!r})")
    assert worst > 0.0          # (the values are not exact: the bound is not idle)


def test_a_face_placed_at_the_default_position_equals_the_file_added_plainly(vg):
    fonts = [(G.variable_glyf_fira("shear"), [0]), (G.variable_glyf_fira("two_axes"), [0, 0]), (G.edge_faces()["inference"][0], [0]),
             (G.edge_faces()["composites"][0], [0])]
    for font, coords in fonts:
        a, fa = _placed(vg, font, coords=coords, name="Same")
        b = vg.FontManager(False)
        fb = b.add_font_data("Same", font)
        oa, ob = a.record_outlines(fa), b.record_outlines(fb)
        for k in ("cmd_off", "cmds", "scale", "shift_x", "ids", "advances"):
            assert G.bits(oa[k]) == G.bits(ob[k]), k
        G.same_family(a.family_desc(fa), b.family_desc(fb))
        ca, cb = a.command_font_desc(fa), b.command_font_desc(fb)
        for key in TABLE_KEYS:
            assert G.bits(ca[key]) == G.bits(cb[key]), key


def test_a_placed_glyf_face_is_a_command_face_for_every_form(vg):
    font = G.variable_glyf_fira("shear")
    mgr, fid = _placed(vg, font, {"wght": 650})
    # no glyf form: parts, the resident table, the tables for the device's builder
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.record_glyf_parts(fid)
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.resident_font_desc(fid, 0)
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.record_resident(fid)
    assert mgr.font_tables_desc(fid, 0) is None
    with pytest.raises(RuntimeError):
        mgr.charstring_font_desc(fid, 0)
    with pytest.raises(RuntimeError):
        mgr.charstring2_font_desc(fid, 0)
    # ... and the command forms take it: by glyph id, with the table of the position
    r = mgr.record_resident_commands(fid)
    assert len(r["glyph_id"]) > 250
    # the same file added plainly keeps every glyf form, also beside the instance under one name
    plain = vg.FontManager(False)
    pid = plain.add_font_data("Plain", font)
    assert len(plain.record_glyf_parts(pid)["parts"]) > 250 and plain.font_tables_desc(pid, 0) is not None
    mgr.add_font_data("Inst", font)
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.record_glyf_parts(fid)
    assert mgr.font_tables_desc(fid, 1) is not None


def test_faces_that_are_refused(vg):
    for case, font in G.unreadable_gvars().items():
        mgr = vg.FontManager(False)
        with pytest.raises(RuntimeError, match="glyf.*gvar"):
            mgr.add_font_instance_normalized("x", font, [0] * (2 if case == "two_axes_file" else 1))
        assert mgr.font_ids() == []
        mgr.add_font_data("x", font)                                   # the file itself is fine
    font = G.edge_faces()["tuple_counts"][0]
    mgr = vg.FontManager(False)
    with pytest.raises(RuntimeError, match="number of coordinates"):
        mgr.add_font_instance_normalized("x", font, [0, 0])
    with pytest.raises(RuntimeError, match="no such axis"):
        mgr.add_font_instance("x", font, {"wdth": 0.5})
    assert mgr.add_font_instance("x", font, {"wght": 0.5}) == "x" and mgr.font_position("x") == [8192]


def test_without_hvar_the_hmtx_advance_stands(vg):
    """the hand-written faces have no HVAR: advances at a position are those of hmtx (phantom points are not read for them)"""
    font = G.edge_faces()["inference"][0]
    mgr, fid = _placed(vg, font, coords=[16384], name="Edge")
    n = len(mgr.command_font_desc(fid)["cmd_off"]) - 1
    assert mgr.font_hor_advances(fid).tolist() == [600] * n


def test_instance_to_pbf_with_the_dummy_raster_equals_the_yardstick(oracle, vg):
    """whole path on the CPU: the files of the instance at wght 650 = fontTools' points and widths through the oracle"""
    font = G.variable_glyf_fira("shear")
    mgr = vg.FontManager(True)
    fid = mgr.add_font_instance("Fira Medium", font, {"wght": 650})
    w = vg.DummyWriter()
    mgr.render_glyphs(w, vg.Renderer.new_dummy())
    want = G.yardstick_files(font, {"wght": 650}, fid, oracle, mode=oracle.DUMMY)
    assert len(want) == 256
    for path, data in want.items():
        assert w.files[path] == data, path
    plain = vg.FontManager(True)
    plain.add_font_data("Fira Medium", font)
    w2 = vg.DummyWriter()
    plain.render_glyphs(w2, vg.Renderer.new_dummy())
    assert sum(w2.files[p] != w.files[p] for p in want) >= 1
