"""The family tables of all named instances of a file built in one device call, through the façade
(vg_manager_set_family_tables_batched over vg_manager_set_family_tables_on_device, ranges submissions).

The 315-glyph named-instance files of tests/named_instances_kit.py — with their HVAR, and one with HVAR removed so that the
advances follow gvar's phantom points — are rendered under every combination of the gvar-on-device, gvar-batched and gvar-advances
switches, with the new switch on and off.  The PBF files must be byte-identical between on and off and equal to the yardstick
tests/test_gpu_named_instances.py uses: one vg_manager_add_font_instance per instance record, every device switch off.  The stats
must say who built the tables: with the switch on one batched call per file, the families of every font id with a file of its
own; with it off none.  A font id two records arrive at has two files and keeps the single call."""
import itertools

import pytest

pytest.importorskip("fontTools")

import family_batch_kit as B  # noqa: E402
from conftest import FIRA  # noqa: E402
from family_batch_kit import NI, P  # noqa: E402

pytestmark = pytest.mark.gpu

WHICH = ("shear", "two_axes_no_room", "shear_without_hvar")
COMBOS = list(itertools.product((False, True), repeat=3))       # (gvar on device, gvar batched, gvar advances)


def _file(which):
    if which == "shear_without_hvar":
        return NI.with_instances(P.without_hvar("shear"), NI.ONE_AXIS), NI.ONE_AXIS
    return NI.files()[which]


@pytest.fixture(scope="module")
def files():
    return {which: _file(which) for which in WHICH}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


@pytest.fixture(scope="module")
def yardstick(vg, renderer, files):
    """(which, advances) -> the files of one add_font_instance per record, every device switch off; computed once per key, shared,
    never changed.  (The advances switch moves only the file without HVAR.)"""
    made = {}

    def get(which, advances):
        key = (which, advances and which == "shear_without_hvar")
        if key not in made:
            font, records = files[which]
            mgr = vg.FontManager(True)
            mgr.set_gvar_advances(key[1])
            for name, record in zip(NI.instance_names(vg, font), records):
                mgr.add_font_instance(name, font, record["location"])
            made[key] = _render(vg, mgr, renderer)
        return made[key]
    return get


def _manager(vg, gvar, gvar_batched, advances, batched, mixed=False):
    mgr = vg.FontManager(True)
    mgr.set_gvar_advances(advances)
    mgr.set_gvar_on_device(gvar)
    mgr.set_gvar_batched(gvar_batched)
    mgr.set_resident_commands(1 if mixed else 2)
    if mixed:
        mgr.set_glyf_on_device(True), mgr.set_resident_fonts(True), mgr.set_glyf_tables_on_device(True), mgr.set_mixed_stores(True)
    mgr.set_resident_families(True)
    mgr.set_family_tables_on_device(True)
    mgr.set_family_tables_batched(batched)
    return mgr


def _own_ids(ids):
    return [i for i in ids if ids.count(i) == 1]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "gvar%d_batched%d_advances%d" % tuple(map(int, c)))
def test_the_files_do_not_depend_on_the_switch_and_the_stats_say_who_built_the_tables(vg, renderer, files, yardstick, which, combo):
    gvar, gvar_batched, advances = combo
    font, records = files[which]
    want = yardstick(which, advances)
    got = {}
    for batched in (True, False):
        mgr = _manager(vg, gvar, gvar_batched, advances, batched)
        ids = mgr.add_font_named_instances(font)
        got[batched] = _render(vg, mgr, renderer)
        assert got[batched] == want, (which, combo, batched)
        # (equality of real renders: every block of every id is there, and the instances' glyphs are in them)
        assert len(want) == 256 * len(set(ids)) and sum(len(b) for b in want.values()) > 100000 * len(set(ids))
        own, merged = _own_ids(ids), set(ids) - set(_own_ids(ids))
        assert mgr.family_stats()["groups"] > 0                                       # ranges submissions
        tables = mgr.family_table_stats()
        assert tables["built_on_device"] == len(set(ids)) and tables["fallbacks"] == 0
        # one call for the file (one device lane), the families of the ids with a file of their own; a merged id the single way
        assert mgr.family_batch_stats() == ({"calls": 1, "families": len(own)} if batched else {"calls": 0, "families": 0})
        assert len(own) == len(records) - 2 * len(merged) and (which == "two_axes_no_room") == (not merged)
        by_gvar = advances and which == "shear_without_hvar"
        assert mgr.gvar_advance_stats()["device_builds"] == (len(set(ids)) if by_gvar else 0)
        assert mgr.gvar_batch_stats() == ({"calls": 1, "faces": len(records)} if gvar and gvar_batched else {"calls": 0, "faces": 0})
        # the families stay: a second render builds nothing and calls nothing
        assert _render(vg, mgr, renderer) == got[batched]
        assert mgr.family_batch_stats() == {"calls": 0, "families": 0} and mgr.family_table_stats()["built_on_device"] == 0
    assert got[True] == got[False]
    if which == "shear_without_hvar" and combo == (False, False, True):               # the phantom advances do move the files
        assert want != yardstick(which, False)


@pytest.mark.parametrize("which", ["shear", "shear_without_hvar"])
def test_beside_a_glyf_file_the_families_are_mixed_ones(vg, renderer, files, yardstick, which):
    """a static glyf file in the same run: its groups mix glyf and command stores, and an instance's family in such a group is of
    the mixed kind (vgsdf_families_create_tables_mixed)"""
    font, records = files[which]
    want = yardstick(which, True)
    got = {}
    for batched in (True, False):
        mgr = _manager(vg, True, True, True, batched, mixed=True)
        ids = mgr.add_font_named_instances(font)
        mgr.add_font_data("Static Beside", FIRA.read_bytes())
        got[batched] = _render(vg, mgr, renderer)
        assert {p: b for p, b in got[batched].items() if p in want} == want
        assert mgr.mixed_stats()["glyf_fonts"] >= 1 and mgr.family_table_stats()["fallbacks"] == 0
        stats = mgr.family_batch_stats()
        if batched:
            assert stats["calls"] >= 1 and stats["families"] >= len(_own_ids(ids))
        else:
            assert stats == {"calls": 0, "families": 0}
    assert got[True] == got[False]


def test_instances_added_one_by_one_keep_their_own_calls(vg, renderer, files, yardstick):
    font, records = files["two_axes_no_room"]
    mgr = _manager(vg, True, True, False, True)
    for name, record in zip(NI.instance_names(vg, font), records):
        mgr.add_font_instance(name, font, record["location"])
    assert _render(vg, mgr, renderer) == yardstick("two_axes_no_room", False)
    assert mgr.family_batch_stats() == {"calls": 0, "families": 0} and mgr.family_table_stats()["built_on_device"] == len(records)
    assert B.E_ARG == -1
