"""Which submission form takes a group, for every combination of the façade's switches.

A group of blocks reaches the device in one of six forms: the host reader's packed commands, `glyf` parts, glyphs named against
resident glyf stores or against command stores, code-point ranges of families over either kind of store.  The façade tries them in
a fixed order; `expected_form` below is that order, and the counters the façade exports say which one a group became.  Every font
set here is below 3000 glyphs, so a render is one group and every counter is 0 or 1.  Whatever the form, the files are the same
bytes.  (The fall-through when a store does not fit or a decoder refuses is covered where those features are tested.)
"""
import hashlib
import itertools
import json

import pytest

from conftest import FIRA, GOLDEN
from fira_cff_kit import fira_cff_part_file  # noqa: F401  (fixture)
from test_golden_cpu import set_paths

pytestmark = pytest.mark.gpu

SETS = ("glyf", "cff", "both")
# (glyf_on_device, resident_fonts, resident_commands, resident_families)
SWITCHES = list(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1)))
ALL_OFF = (0, 0, 0, 0)
GOLDEN_FIRA = json.loads((GOLDEN / "pbf_sha256.json").read_text())["fira"]


def expected_form(all_glyf, glyf_on_device, resident_fonts, commands, families):
    """all_glyf: every glyph of the group comes from a `glyf` file"""
    by_name_or_range = "ranges_{}" if families else "named_{}"
    if commands == 2:
        return by_name_or_range.format("commands")
    if glyf_on_device and all_glyf:
        return by_name_or_range.format("glyf") if resident_fonts else "glyf_parts"
    if commands == 1:
        return by_name_or_range.format("commands")
    return "packed"


# the one counter a form raises (ranges are counted as family groups and not among the named ones)
COUNTER_OF = {"ranges_commands": "family", "ranges_glyf": "family", "named_glyf": "resident", "named_commands": "command",
              "glyf_parts": "glyf", "packed": None}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def sources(fira_cff_part_file):
    return {"glyf": [FIRA], "cff": [fira_cff_part_file], "both": [fira_cff_part_file, FIRA]}


def _render(vg, renderer, paths, switches):
    glyf_on_device, resident_fonts, commands, families = switches
    mgr = vg.FontManager(True)
    mgr.set_glyf_on_device(bool(glyf_on_device))
    mgr.set_resident_fonts(bool(resident_fonts))
    mgr.set_resident_commands(commands)
    mgr.set_resident_families(bool(families))
    mgr.add_font_with_name(set_paths("fira")[0], paths)
    w = vg.DummyWriter()
    mgr.render_glyphs(w, renderer)
    return mgr, w.files


@pytest.fixture(scope="module")
def plain(vg, renderer, sources):
    """the files of every font set with all four switches off: rendered once, compared against by every case"""
    return {which: _render(vg, renderer, sources[which], ALL_OFF)[1] for which in SETS}


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "glyf%d-fonts%d-commands%d-families%d" % s)
@pytest.mark.parametrize("which", SETS)
def test_the_form_a_group_takes_and_its_bytes(vg, renderer, sources, plain, which, switches):
    mgr, files = _render(vg, renderer, sources[which], switches)
    t = mgr.timings()
    assert 0 < t["glyphs"] < 3000 and t["fe_groups"] == 1 and t["glyf_fallbacks"] == 0
    got = {"family": mgr.family_stats()["groups"], "resident": mgr.resident_stats()["groups"],
           "command": mgr.command_stats()["groups"], "glyf": t["glyf_groups"]}
    form = expected_form(which == "glyf", *switches)
    want = dict.fromkeys(got, 0)
    if COUNTER_OF[form]:
        want[COUNTER_OF[form]] = 1
    assert got == want, form
    assert files == plain[which]
    if which == "glyf":
        assert {k.split("/", 1)[1].split("-")[0]: hashlib.sha256(v).hexdigest() for k, v in files.items()} == GOLDEN_FIRA
