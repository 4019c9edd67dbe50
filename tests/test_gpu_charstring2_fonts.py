"""CFF2 charstrings on the device through the façade (vg_manager_set_charstrings_on_device with the value 2): the command store
of a `CFF2` face is decoded by the device (vgsdf_font_create_charstrings2, the reader's blend factors) instead of built by the
host's reader, and every file the render writes is, byte for byte, the file the same render writes with the switch off.  With the
value 1 a CFF2 face is left to the host's reader, and a `CFF ` version 1 face behaves with 2 as it does with 1."""
import pytest

pytest.importorskip("fontTools")

import charstring2_edge_programs as K2  # noqa: E402
from fira_cff_kit import fira_as_cff  # noqa: E402
from test_cff2_outlines import _variable_fira  # noqa: E402

pytestmark = pytest.mark.gpu

NO_CHARSTRINGS = {"fonts_decoded": 0, "font_bytes": 0, "fallbacks": 0}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def fira_cff2():
    return _variable_fira()


def _manager(vg, font, on, families=False, mode=1):
    mgr = vg.FontManager(True)
    mgr.set_resident_commands(mode)
    mgr.set_charstrings_on_device(on)
    mgr.set_resident_families(families)
    mgr.add_font_data("Face", font)
    return mgr


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


@pytest.mark.parametrize("families", [False, True], ids=["by_glyph_id", "families"])
@pytest.mark.parametrize("mode", [1, 2], ids=["commands_1", "commands_2"])
def test_the_files_do_not_depend_on_who_decodes_the_cff2_charstrings(vg, renderer, fira_cff2, mode, families):
    off = _manager(vg, fira_cff2, 0, families, mode)
    want = _render(vg, off, renderer)
    assert len(want) >= 1 and off.charstring_stats() == NO_CHARSTRINGS and off.command_stats()["fonts_uploaded"] == 1
    # 1: `CFF ` version 1 faces only — the CFF2 face is not decoded on the device
    one = _manager(vg, fira_cff2, 1, families, mode)
    assert _render(vg, one, renderer) == want
    assert one.charstring_stats() == NO_CHARSTRINGS and one.command_stats()["fonts_uploaded"] == 1
    on = _manager(vg, fira_cff2, 2, families, mode)
    got = _render(vg, on, renderer)
    assert got == want
    s, c = on.charstring_stats(), on.command_stats()
    assert s["fonts_decoded"] == 1 and s["fallbacks"] == 0 and s["font_bytes"] == c["font_bytes"] == off.command_stats()["font_bytes"] > 0
    assert c["fonts_uploaded"] == 1
    # the store stays: the second render decodes nothing
    assert _render(vg, on, renderer) == want and on.charstring_stats() == NO_CHARSTRINGS and on.command_stats()["fonts_uploaded"] == 0


def test_true_still_means_1(vg, renderer, fira_cff2):
    mgr = _manager(vg, fira_cff2, True)
    _render(vg, mgr, renderer)
    assert mgr.charstring_stats() == NO_CHARSTRINGS and mgr.command_stats()["fonts_uploaded"] == 1


def test_a_version_1_face_behaves_with_2_as_with_1(vg, renderer):
    font = fira_as_cff(300)
    want = _render(vg, _manager(vg, font, 0), renderer)
    stats = {}
    for on in (1, 2):
        mgr = _manager(vg, font, on)
        assert _render(vg, mgr, renderer) == want
        stats[on] = (mgr.charstring_stats(), mgr.command_stats())
        assert stats[on][0]["fonts_decoded"] == 1 and stats[on][0]["fallbacks"] == 0
    assert stats[1] == stats[2]


def test_a_glyph_past_the_token_budget_sends_the_face_back_to_the_host_reader(vg, renderer):
    font = K2.budget_faces()[1].font()
    want = _render(vg, _manager(vg, font, 0), renderer)
    assert len(want) >= 1
    on = _manager(vg, font, 2)
    assert _render(vg, on, renderer) == want
    assert on.charstring_stats() == {"fonts_decoded": 0, "font_bytes": 0, "fallbacks": 1} and on.command_stats()["fonts_uploaded"] == 1
    # the refusal is remembered: no second attempt, no second fallback
    assert _render(vg, on, renderer) == want and on.charstring_stats() == NO_CHARSTRINGS


def test_mode_0_and_preload(vg, fira_cff2):
    r = vg.Renderer.new_precise(0)
    mgr = _manager(vg, fira_cff2, 2, mode=0)
    _render(vg, mgr, r)
    assert mgr.charstring_stats() == NO_CHARSTRINGS
    sizes = {}
    for on in (0, 2):
        r = vg.Renderer.new_precise(0)
        mgr = _manager(vg, fira_cff2, on)
        sizes[on] = r.preload_fonts(mgr)
        assert mgr.charstring_preload_stats() == {"fonts_decoded": int(on == 2), "font_bytes": sizes[on] if on else 0, "fallbacks": 0}
    assert sizes[0] == sizes[2] > 0
