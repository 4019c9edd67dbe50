"""The façade's mixed stores (vg_manager_set_mixed_stores): which form a group takes for every combination of the switches with the
new one on, what the counters say, and that the files are the same bytes.

The font sets are those of tests/test_gpu_group_forms.py — `glyf` (Fira Sans), `cff` (its first 400 glyph ids re-encoded as CFF)
and `both` (the CFF file in front of Fira Sans under ONE font id) — and `two_ids`, a manager with a glyf font id and a CFF font id
in one group.  `expected_form` below states the order with the switch on; with it off every form and counter is as
test_gpu_group_forms.py states.  Every set is small enough to be one group of the dispatcher, so every group counter is 0 or 1.
The files of every case equal those rendered with all switches off; for `glyf` the golden SHAs are checked as well.
"""
import hashlib
import itertools
import json

import pytest

import mixed_kinds_kit as M
from conftest import FIRA, GOLDEN
from fira_cff_kit import fira_cff_part_file  # noqa: F401  (fixture)
from test_golden_cpu import set_paths
from test_gpu_group_forms import expected_form as form_without_the_switch

pytestmark = pytest.mark.gpu

SETS = ("glyf", "cff", "both", "two_ids")
# (glyf_on_device, resident_fonts, resident_commands, resident_families)
SWITCHES = list(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1)))
ALL_OFF = (0, 0, 0, 0)
GOLDEN_FIRA = json.loads((GOLDEN / "pbf_sha256.json").read_text())["fira"]
N_FILES = {"glyf": 1, "cff": 1, "both": 2, "two_ids": 2}
ZERO = {"groups": 0, "glyf_fonts": 0, "command_fonts": 0, "block_bytes": 0}


def expected_form(which, glyf_on_device, resident_fonts, commands, families):
    """the form with the new switch ON"""
    by_name_or_range = "ranges_{}" if families else "named_{}"
    all_glyf, a_glyf_file = which == "glyf", which != "cff"
    if commands == 2:
        return by_name_or_range.format("commands")
    if glyf_on_device and all_glyf:
        return by_name_or_range.format("glyf") if resident_fonts else "glyf_parts"
    if glyf_on_device and resident_fonts and commands == 1 and a_glyf_file:
        return by_name_or_range.format("mixed")
    return form_without_the_switch(all_glyf, glyf_on_device, resident_fonts, commands, families)


COUNTER_OF = {"ranges_commands": "family", "ranges_glyf": "family", "named_glyf": "resident", "named_commands": "command",
              "glyf_parts": "glyf", "packed": None, "ranges_mixed": "mixed", "named_mixed": "mixed"}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def sources(fira_cff_part_file):
    fira = set_paths("fira")[0]
    return {"glyf": [(fira, [FIRA])], "cff": [(fira, [fira_cff_part_file])], "both": [(fira, [fira_cff_part_file, FIRA])],
            "two_ids": [(fira, [FIRA]), ("Fira Sans CFF Regular", [fira_cff_part_file])]}


def _manager(vg, fonts, switches, mixed, in_place=True, builders=False):
    glyf_on_device, resident_fonts, commands, families = switches
    mgr = vg.FontManager(True)
    mgr.set_glyf_on_device(bool(glyf_on_device))
    mgr.set_resident_fonts(bool(resident_fonts))
    mgr.set_resident_commands(commands)
    mgr.set_resident_families(bool(families))
    if mixed is not None:
        mgr.set_mixed_stores(mixed)
    mgr.set_in_place_pbf(in_place)
    if builders:
        mgr.set_glyf_tables_on_device(True)
        mgr.set_charstrings_on_device(1)
        mgr.set_family_tables_on_device(True)
    for name, paths in fonts:
        mgr.add_font_with_name(name, paths)
    return mgr


def _render(vg, renderer, mgr):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, renderer)
    return w.files


def _group_counters(mgr):
    return {"family": mgr.family_stats()["groups"], "resident": mgr.resident_stats()["groups"], "command": mgr.command_stats()["groups"],
            "glyf": mgr.timings()["glyf_groups"], "mixed": mgr.mixed_stats()["groups"]}


@pytest.fixture(scope="module")
def plain(vg, renderer, sources):
    """the files of every font set with every switch off: rendered once, compared against by every case"""
    return {which: _render(vg, renderer, _manager(vg, sources[which], ALL_OFF, None)) for which in SETS}


def _assert_the_one_group(mgr, which, form):
    t = mgr.timings()
    assert 0 < t["glyphs"] < 3000 + 3000 * (which == "two_ids") and t["fe_groups"] == 1 and t["glyf_fallbacks"] == 0
    want = dict.fromkeys(("family", "resident", "command", "glyf", "mixed"), 0)
    if COUNTER_OF[form]:
        want[COUNTER_OF[form]] = 1
    assert _group_counters(mgr) == want, form
    mixed = mgr.mixed_stats()
    if form == "named_mixed":          # the glyf form's block: 33 bytes per glyph + 8, 16-aligned, and 32 per store
        assert mixed == {"groups": 1, "glyf_fonts": 1, "command_fonts": 1, "block_bytes": M.upload_bytes(t["glyphs"], N_FILES[which], True)}
    elif form == "ranges_mixed":       # 32 bytes per task that maps a glyph, per family and per store: nothing per glyph
        assert (mixed["groups"], mixed["glyf_fonts"], mixed["command_fonts"]) == (1, 1, 1)
        n_families = 2 if which == "two_ids" else 1
        assert mixed["block_bytes"] % 32 == 0 and 32 * (1 + n_families + N_FILES[which]) <= mixed["block_bytes"] <= 32 * (256 * n_families + 4)
    else:
        assert mixed == ZERO


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "glyf%d-fonts%d-commands%d-families%d" % s)
@pytest.mark.parametrize("which", SETS)
def test_the_form_a_group_takes_with_the_switch_on(vg, renderer, sources, plain, which, switches):
    mgr = _manager(vg, sources[which], switches, True)
    files = _render(vg, renderer, mgr)
    _assert_the_one_group(mgr, which, expected_form(which, *switches))
    assert files == plain[which]
    if which == "glyf":
        assert {k.split("/", 1)[1].split("-")[0]: hashlib.sha256(v).hexdigest() for k, v in files.items()} == GOLDEN_FIRA


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "glyf%d-fonts%d-commands%d-families%d" % s)
@pytest.mark.parametrize("which", ["both", "two_ids"])
def test_with_the_switch_off_every_form_is_as_before(vg, renderer, sources, plain, which, switches):
    mgr = _manager(vg, sources[which], switches, False)
    files = _render(vg, renderer, mgr)
    _assert_the_one_group(mgr, which, form_without_the_switch(False, *switches))
    assert files == plain[which]


@pytest.mark.parametrize("families", [0, 1])
@pytest.mark.parametrize("which", ["both", "two_ids"])
def test_the_glyf_file_is_not_turned_into_commands(vg, sources, plain, which, families):
    """a fresh renderer per mode: with the switch on the group names one glyf store and ONE command store — Fira's glyf file got
    no command store; with it off the same set uploads two.  A second render uploads nothing"""
    switches = (1, 1, 1, families)
    r = vg.Renderer.new_precise(0)
    try:
        mgr = _manager(vg, sources[which], switches, True)
        assert _render(vg, r, mgr) == plain[which]
        mixed = mgr.mixed_stats()
        assert (mixed["groups"], mixed["glyf_fonts"], mixed["command_fonts"]) == (1, 1, 1)
        assert mgr.command_stats()["fonts_uploaded"] == 1 and mgr.resident_stats()["fonts_uploaded"] == 1
        # one mixed family per font id (two_ids: the blocks behind the run's last glyph form a group of their own without a glyph,
        # all of the glyf font id, which is recorded against that id's glyf family as it is without the switch)
        assert mgr.family_stats()["families_uploaded"] == (0 if not families else 2 + 1 if which == "two_ids" else 1)
        assert _render(vg, r, mgr) == plain[which]
        assert mgr.mixed_stats() == mixed
        assert mgr.command_stats()["fonts_uploaded"] == 0 and mgr.resident_stats()["fonts_uploaded"] == 0
        assert mgr.family_stats()["families_uploaded"] == 0
    finally:
        r.close()
    r = vg.Renderer.new_precise(0)
    try:
        mgr = _manager(vg, sources[which], switches, False)
        assert _render(vg, r, mgr) == plain[which]
        assert mgr.mixed_stats() == ZERO and mgr.command_stats()["fonts_uploaded"] == 2
    finally:
        r.close()


@pytest.mark.parametrize("families", [0, 1])
def test_every_device_builder_on(vg, sources, plain, families):
    """glyf tables, charstrings and family tables built on the device: each builder built its one store / family and none fell
    back"""
    r = vg.Renderer.new_precise(0)
    try:
        mgr = _manager(vg, sources["both"], (1, 1, 1, families), True, builders=True)
        assert _render(vg, r, mgr) == plain["both"]
        _assert_the_one_group(mgr, "both", "ranges_mixed" if families else "named_mixed")
        g, c, f = mgr.glyf_table_stats(), mgr.charstring_stats(), mgr.family_table_stats()
        assert g["built_on_device"] == 1 and g["fallbacks"] == 0
        assert c["fonts_decoded"] == 1 and c["fallbacks"] == 0
        assert f == {"built_on_device": families, "fallbacks": 0}
        assert mgr.command_stats()["fonts_uploaded"] == 1 and mgr.resident_stats()["fonts_uploaded"] == 1
    finally:
        r.close()


@pytest.mark.parametrize("families", [0, 1])
@pytest.mark.parametrize("which", ["both", "two_ids"])
def test_in_place_pbf_off(vg, renderer, sources, plain, which, families):
    mgr = _manager(vg, sources[which], (1, 1, 1, families), True, in_place=False)
    assert _render(vg, renderer, mgr) == plain[which]
    t, mixed = mgr.timings(), mgr.mixed_stats()
    assert (mixed["groups"], mixed["glyf_fonts"], mixed["command_fonts"]) == (1, 1, 1) and t["fe_groups"] == 1
    if not families:
        assert mixed["block_bytes"] == M.upload_bytes(t["glyphs"], 2, False)


@pytest.mark.parametrize("families", [0, 1])
def test_preloading_builds_the_stores_and_the_mixed_families(vg, sources, plain, families):
    r = vg.Renderer.new_precise(0)
    try:
        mgr = _manager(vg, sources["both"], (1, 1, 1, families), True)
        assert r.preload_fonts(mgr) > 0 and r.preload_fonts(mgr) == 0
        assert _render(vg, r, mgr) == plain["both"]
        assert mgr.mixed_stats()["groups"] == 1
        assert mgr.family_stats()["families_uploaded"] == 0 and mgr.command_stats()["fonts_uploaded"] == 0
        assert mgr.resident_stats()["fonts_uploaded"] == 0
    finally:
        r.close()


@pytest.mark.parametrize("families", [0, 1])
def test_two_lanes_on_device_0(vg, sources, plain, families):
    """the hybrid lane plan on {0, 0}: every lane's groups take the form their own glyphs allow — mixed where a lane's group
    holds glyphs of both files — and the lanes share the stores and the family"""
    r = vg.Renderer.new_multi([0, 0])
    try:
        mgr = _manager(vg, sources["both"], (1, 1, 1, families), True)
        mgr.set_lane_form(2)
        assert _render(vg, r, mgr) == plain["both"]
        t, got = mgr.timings(), _group_counters(mgr)
        assert got["mixed"] >= 1 and sum(got.values()) == t["fe_groups"] >= 2 and t["glyf_fallbacks"] == 0
        assert got["command"] + got["family"] + got["resident"] + got["glyf"] + got["mixed"] == t["fe_groups"]
        assert mgr.command_stats()["fonts_uploaded"] == 1 and mgr.resident_stats()["fonts_uploaded"] == 1
        assert _render(vg, r, mgr) == plain["both"]
        assert mgr.command_stats()["fonts_uploaded"] == 0 and mgr.family_stats()["families_uploaded"] == 0
    finally:
        r.close()
