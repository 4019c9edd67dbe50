"""All CFF2 instances of a file in one device build, through the façade (vg_manager_set_charstrings_batched over
vg_manager_set_charstrings_on_device(m, 2)).

The named instances of the variable CFF2 Fira fixtures — nine weights on one axis, three positions on two — are rendered with the
switch on and off under the combinations of resident commands, resident families, family tables on the device and batched family
tables that tests/test_gpu_family_batch_fonts.py walks.  The files must be the same bytes on and off, equal to one
vg_manager_add_font_instance per record with every switch off, and — for the instances at positions where it is valid — to the
independent yardstick of tests/variable_instances_kit.py.  The stats say who built the stores: one batched call per file and all
its faces on the first render, nothing on the second."""
import pytest

pytest.importorskip("fontTools")

import charstring2_batch_kit as B  # noqa: E402
import named_instances_kit as N  # noqa: E402
import variable_instances_kit as V  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = {"calls": 0, "faces": 0}
CONFIGS = [dict(commands=1), dict(commands=2), dict(commands=2, families=True), dict(commands=2, families=True, tables=True),
           dict(commands=2, families=True, tables=True, tables_batched=True), dict(commands=1, families=True, tables=True, tables_batched=True)]


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


def _manager(vg, charstrings=2, batched=False, commands=1, families=False, tables=False, tables_batched=False):
    mgr = vg.FontManager(True)
    mgr.set_charstrings_on_device(charstrings)
    mgr.set_charstrings_batched(batched)
    mgr.set_resident_commands(commands)
    mgr.set_resident_families(families)
    mgr.set_family_tables_on_device(tables)
    mgr.set_family_tables_batched(tables_batched)
    return mgr


@pytest.fixture(scope="module")
def yardsticks(vg, renderer):
    """one add_font_instance per record, every switch off: computed once, shared, never changed"""
    made = {}
    for which in ("one_axis", "two_axes"):
        font, records = B.instance_files()[which]
        mgr = vg.FontManager(True)
        for name, record in zip(N.instance_names(vg, font), records):
            mgr.add_font_instance(name, font, record["location"])
        made[which] = _render(vg, mgr, renderer)
    return made


def test_the_yardstick_equals_the_independent_one_where_that_is_valid(vg, oracle, yardsticks):
    font, _ = B.instance_files()["one_axis"]
    want = V.yardstick_files(font, {"wght": 650}, "synth_var_semibold", oracle)
    assert len(want) == 256 and all(yardsticks["one_axis"][p] == b for p, b in want.items())
    font, _ = B.instance_files()["two_axes"]
    want = V.yardstick_files(font, {"wght": 650, "wdth": 100}, "synth_var_medium", oracle)
    assert len(want) == 256 and all(yardsticks["two_axes"][p] == b for p, b in want.items())


@pytest.mark.parametrize("which", ["one_axis", "two_axes"])
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "_".join(f"{k}{int(v)}" for k, v in c.items()))
def test_the_files_do_not_depend_on_the_switch_and_the_stats_say_who_built_the_stores(vg, renderer, yardsticks, which, config):
    font, records = B.instance_files()[which]
    n = len(records)
    got = {}
    for batched in (True, False):
        mgr = _manager(vg, batched=batched, **config)
        assert len(set(mgr.add_font_named_instances(font))) == n
        got[batched] = _render(vg, mgr, renderer)
        assert got[batched] == yardsticks[which], (which, config, batched)
        assert len(got[batched]) == 256 * n
        cs = mgr.charstring_stats()
        assert cs["fonts_decoded"] == n and cs["fallbacks"] == 0 and cs["font_bytes"] > 0
        assert mgr.command_stats()["fonts_uploaded"] == n
        assert mgr.charstring_batch_stats() == ({"calls": 1, "faces": n} if batched else NONE)
        if config.get("tables_batched"):
            assert mgr.family_batch_stats() == {"calls": 1, "families": n}
        # the stores stay: a second render builds nothing and calls nothing
        assert _render(vg, mgr, renderer) == got[batched]
        assert mgr.charstring_batch_stats() == NONE and mgr.charstring_stats()["fonts_decoded"] == 0
    assert got[True] == got[False]


def test_the_switch_acts_only_with_cff2_charstrings_on_the_device(vg, renderer, yardsticks):
    font, records = B.instance_files()["two_axes"]
    for charstrings in (0, 1):
        mgr = _manager(vg, charstrings=charstrings, batched=True, commands=2)
        mgr.add_font_named_instances(font)
        assert _render(vg, mgr, renderer) == yardsticks["two_axes"]
        assert mgr.charstring_batch_stats() == NONE and mgr.charstring_stats()["fonts_decoded"] == 0


def test_preloading_builds_the_stores_of_a_group_in_one_call(vg, yardsticks):
    font, records = B.instance_files()["one_axis"]
    r = vg.Renderer.new_precise(0)
    mgr = _manager(vg, batched=True, commands=2)
    mgr.add_font_named_instances(font)
    assert r.preload_fonts(mgr) > 0
    assert mgr.charstring_preload_stats()["fonts_decoded"] == len(records) and mgr.charstring_preload_stats()["fallbacks"] == 0
    assert _render(vg, mgr, r) == yardsticks["one_axis"]
    assert mgr.command_stats()["fonts_uploaded"] == 0 and mgr.charstring_batch_stats() == NONE        # all there already
    assert mgr.charstring_stats()["fonts_decoded"] == 0


def test_a_group_of_one_and_files_added_one_by_one_keep_the_single_path(vg, renderer, yardsticks):
    font, records = B.instance_files()["two_axes"]
    mgr = _manager(vg, batched=True, commands=2)
    for name, record in zip(N.instance_names(vg, font), records):
        mgr.add_font_instance(name, font, record["location"])
    assert _render(vg, mgr, renderer) == yardsticks["two_axes"]
    assert mgr.charstring_stats()["fonts_decoded"] == len(records) and mgr.charstring_batch_stats() == NONE
    # a file with one instance record: a group of one
    one = N.with_instances(V.variable_fira(120, two_axes=True), N.TWO_AXES[:1], room_for_ps=False)
    mgr = _manager(vg, batched=True, commands=2)
    ids = mgr.add_font_named_instances(one)
    assert len(ids) == 1 and mgr.instance_group(ids[0]) == ids
    got = _render(vg, mgr, renderer)
    assert got == {p: b for p, b in yardsticks["two_axes"].items() if p.startswith(ids[0] + "/")}
    assert mgr.charstring_stats()["fonts_decoded"] == 1 and mgr.charstring_batch_stats() == NONE
