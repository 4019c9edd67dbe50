"""Charstrings on the device through the façade (vg_manager_set_charstrings_on_device): the command stores of `CFF ` faces are
decoded by the device instead of built by the host's reader, and every file the render writes is, byte for byte, the file the
same render writes with the switch off."""
import pytest

pytest.importorskip("fontTools")
from fontTools.misc.psCharStrings import T2CharString  # noqa: E402

import charstring_edge_programs as K  # noqa: E402
from test_cff_outlines import _build, fira_cff, ops_cff  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

NO_CHARSTRINGS = {"fonts_decoded": 0, "font_bytes": 0, "fallbacks": 0}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def cid_font():
    return K.cid_face().font()


@pytest.fixture(scope="module")
def seac_font():
    """tests/test_cff_outlines.py's accented glyphs: base and accent through the charset, drawn by the HOST reader only"""
    names = [".notdef", "A", "acute", "Aacute", "dieresis", "Adieresis", "o", "oacute"]
    progs = [
        [0, "hmoveto", "endchar"],
        [600, 100, 0, "rmoveto", 200, 700, "rlineto", 200, -700, "rlineto", "endchar"],
        [300, 10, 20, "hstem", 50, 60, "rmoveto", 80, 120, "rlineto", -40, 0, "rlineto", "endchar"],
        [640, 150, 700, 65, 194, "endchar"],
        [250, 0, "rmoveto", 60, "hlineto", 60, "vlineto", -60, "hlineto", 100, 0, "rmoveto", 60, "hlineto", 60, "vlineto", -60, "hlineto", "endchar"],
        [100, 720, 65, 200, "endchar"],
        [550, 100, 100, "rmoveto", 100, 0, 100, 100, 0, 100, "rrcurveto", -100, 0, -100, -100, 0, -100, "rrcurveto", "endchar"],
        [-20, 520, 111, 194, "endchar"],
    ]
    cs = {n: T2CharString(program=list(p)) for n, p in zip(names, progs)}
    cmap = {0x41: "A", 0xB4: "acute", 0xC1: "Aacute", 0xA8: "dieresis", 0xC4: "Adieresis", 0x6F: "o", 0xF3: "oacute"}
    return _build(names, cmap, cs, {n: 600 for n in names})


def _manager(vg, font, on, in_place=True, families=False, mode=1):
    mgr = vg.FontManager(True)
    mgr.set_resident_commands(mode)
    mgr.set_charstrings_on_device(on)
    mgr.set_in_place_pbf(in_place)
    mgr.set_resident_families(families)
    mgr.add_font_data("Face", font)
    return mgr


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


@pytest.mark.parametrize("families", [False, True], ids=["by_glyph_id", "families"])
@pytest.mark.parametrize("in_place", [True, False], ids=["in_place_pbf", "packed_bitmaps"])
@pytest.mark.parametrize("which", ["fira_cff", "ops_cff", "cid_font"])
def test_the_files_do_not_depend_on_who_decodes_the_charstrings(vg, renderer, request, which, in_place, families):
    font = request.getfixturevalue(which)
    off = _manager(vg, font, False, in_place, families)
    want = _render(vg, off, renderer)
    assert len(want) >= 1 and off.charstring_stats() == NO_CHARSTRINGS and off.command_stats()["fonts_uploaded"] == 1
    on = _manager(vg, font, True, in_place, families)
    got = _render(vg, on, renderer)
    assert got == want
    s, c = on.charstring_stats(), on.command_stats()
    assert s["fonts_decoded"] == 1 and s["fallbacks"] == 0 and s["font_bytes"] == c["font_bytes"] == off.command_stats()["font_bytes"] > 0
    assert c["fonts_uploaded"] == 1
    # the store stays: the second render decodes nothing
    assert _render(vg, on, renderer) == want and on.charstring_stats() == NO_CHARSTRINGS and on.command_stats()["fonts_uploaded"] == 0


def test_a_seac_glyph_sends_the_face_back_to_the_host_reader(vg, renderer, seac_font):
    want = _render(vg, _manager(vg, seac_font, False), renderer)
    on = _manager(vg, seac_font, True)
    assert _render(vg, on, renderer) == want
    assert on.charstring_stats() == {"fonts_decoded": 0, "font_bytes": 0, "fallbacks": 1} and on.command_stats()["fonts_uploaded"] == 1
    assert _render(vg, on, renderer) == want and on.charstring_stats() == NO_CHARSTRINGS


def test_mode_0_and_glyf_faces_are_untouched(vg, renderer, fira_cff):  # noqa: F811
    from conftest import FIRA
    mgr = _manager(vg, fira_cff, True, mode=0)
    _render(vg, mgr, renderer)
    assert mgr.charstring_stats() == NO_CHARSTRINGS
    glyf = vg.FontManager(True)
    glyf.set_resident_commands(2)
    glyf.set_charstrings_on_device(True)
    glyf.add_font_with_name("Fira", [FIRA])
    assert len(_render(vg, glyf, renderer)) >= 1
    assert glyf.charstring_stats() == NO_CHARSTRINGS


def test_preload_builds_the_stores_on_the_device(vg, fira_cff):  # noqa: F811
    sizes = {}
    for on in (False, True):
        r = vg.Renderer.new_precise(0)
        mgr = _manager(vg, fira_cff, on)
        sizes[on] = r.preload_fonts(mgr)
        # who built the store: the device's decoder with the switch on, the host reader's table with it off
        assert mgr.charstring_preload_stats() == {"fonts_decoded": int(on), "font_bytes": sizes[on] if on else 0, "fallbacks": 0}
        assert sizes[on] > 0 and r.preload_fonts(mgr) == 0 and mgr.charstring_preload_stats() == NO_CHARSTRINGS
        _render(vg, mgr, r)
        assert mgr.charstring_stats() == NO_CHARSTRINGS and mgr.command_stats()["fonts_uploaded"] == 0
        assert mgr.command_stats()["groups"] >= 1
    assert sizes[True] == sizes[False]


def test_preload_counts_a_refused_face_as_a_fallback(vg, seac_font):
    r = vg.Renderer.new_precise(0)
    mgr = _manager(vg, seac_font, True)
    assert r.preload_fonts(mgr) > 0
    assert mgr.charstring_preload_stats() == {"fonts_decoded": 0, "font_bytes": 0, "fallbacks": 1}


def test_a_store_past_the_budget_is_not_allocated(vg, fira_cff):  # noqa: F811
    """budget 0: the device counts, allocates no store, and the render goes on as with the switch off"""
    r = vg.Renderer.new_precise(0)
    r.set_resident_budget(0)
    want = _render(vg, _manager(vg, fira_cff, False), r)
    on = _manager(vg, fira_cff, True)
    assert _render(vg, on, r) == want
    assert on.charstring_stats() == NO_CHARSTRINGS and on.command_stats()["fonts_uploaded"] == 0


def test_a_face_that_did_not_fit_is_decoded_once_the_budget_has_room(vg, fira_cff):  # noqa: F811
    r = vg.Renderer.new_precise(0)
    r.set_resident_budget(0)
    mgr = _manager(vg, fira_cff, True)
    want = _render(vg, mgr, r)
    assert mgr.charstring_stats() == NO_CHARSTRINGS and mgr.command_stats()["fonts_uploaded"] == 0
    r.set_resident_budget(1 << 30)
    assert _render(vg, mgr, r) == want
    assert mgr.charstring_stats()["fonts_decoded"] == 1 and mgr.charstring_stats()["fallbacks"] == 0
    assert mgr.command_stats()["fonts_uploaded"] == 1 and mgr.command_stats()["groups"] >= 1
