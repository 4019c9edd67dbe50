"""The named instances of a variable `glyf` file rendered through the façade on the GPU (vg_manager_add_font_named_instances).

The yardstick is the path tests/test_gpu_gvar_instances.py holds against an independent one: one vg_manager_add_font_instance per
instance record under the same name, every switch off, the command stores made from the host reader's tables.  The files after
add_font_named_instances must equal those byte for byte whoever builds the stores — the host, the device one face at a time
(vg_manager_set_gvar_on_device), the device one group at a time (vg_manager_set_gvar_batched) — and with resident families, mixed
stores and in-place PBF on and off; the stats must say who did: with batching one call per group, never a glyf form.  A group
with positions the device refuses: those ids fall back to the host's table, once, and the files are still equal."""
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
import named_instances_kit as N  # noqa: E402

pytestmark = pytest.mark.gpu

NO_GLYF_WORK = {"built_on_device": 0, "bytes": 0, "fallbacks": 0}
MODES = {"host": dict(gvar=False, batched=False), "device": dict(gvar=True, batched=False), "device_batched": dict(gvar=True, batched=True),
         "batched_alone": dict(gvar=False, batched=True)}
CONFIGS = [dict(commands=1), dict(commands=2, families=True, tables=True), dict(glyf=True, commands=1, mixed=True),
           dict(glyf=True, commands=1, mixed=True, families=True, tables=True), dict(commands=1, in_place=False)]


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


def _manager(vg, glyf=False, commands=1, mixed=False, families=False, tables=False, in_place=True, gvar=False, batched=False):
    mgr = vg.FontManager(True)
    mgr.set_gvar_on_device(gvar)
    mgr.set_gvar_batched(batched)
    mgr.set_glyf_on_device(glyf)
    mgr.set_resident_fonts(glyf)
    mgr.set_glyf_tables_on_device(glyf)
    mgr.set_resident_commands(commands)
    mgr.set_mixed_stores(mixed)
    mgr.set_resident_families(families)
    mgr.set_family_tables_on_device(tables)
    mgr.set_in_place_pbf(in_place)
    return mgr


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


def _one_instance_per_record(vg, renderer, font, records):
    mgr = vg.FontManager(True)
    for name, record in zip(N.instance_names(vg, font), records):
        mgr.add_font_instance(name, font, record["location"])
    assert mgr.font_ids() == sorted(set(N.instance_ids(vg, font)))
    return _render(vg, mgr, renderer)


@pytest.fixture(scope="module")
def yardsticks(vg, renderer):
    """computed once, shared, never changed"""
    return {which: _one_instance_per_record(vg, renderer, *N.files()[which]) for which in ("shear", "two_axes_no_room")}


def test_with_every_switch_off_the_files_are_those_of_one_add_per_record(vg, renderer, yardsticks):
    for which, want in yardsticks.items():
        font, records = N.files()[which]
        mgr = vg.FontManager(True)
        ids = mgr.add_font_named_instances(font)
        got = _render(vg, mgr, renderer)
        assert got == want and len(got) == 256 * len(set(ids))
        assert mgr.gvar_batch_stats() == {"calls": 0, "faces": 0}
    # the positions matter: the instances' files differ from one another
    medium = {p.split("/", 1)[1]: b for p, b in yardsticks["two_axes_no_room"].items() if p.startswith("synth_gvar_medium/")}
    black = {p.split("/", 1)[1]: b for p, b in yardsticks["two_axes_no_room"].items() if p.startswith("synth_gvar_black/")}
    assert len(medium) == len(black) == 256 and sum(medium[p] != black[p] for p in medium) >= 1


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "_".join(f"{k}{int(v)}" for k, v in c.items()))
def test_the_files_do_not_depend_on_who_builds_the_stores(vg, renderer, yardsticks, config, mode):
    gvar, batched = MODES[mode]["gvar"], MODES[mode]["batched"]
    for which, want in yardsticks.items():
        font, records = N.files()[which]
        mgr = _manager(vg, **config, **MODES[mode])
        mgr.add_font_named_instances(font)
        got = _render(vg, mgr, renderer)
        assert got == want, (which, config, mode)
        # never a glyf form: no glyf store is built or uploaded, no group names one
        assert mgr.glyf_table_stats() == NO_GLYF_WORK and mgr.resident_stats()["fonts_uploaded"] == 0
        assert mgr.mixed_stats()["glyf_fonts"] == 0
        n = len(records)
        assert mgr.command_stats()["fonts_uploaded"] == n
        built = mgr.gvar_stats()
        assert built["fonts_built"] == (n if gvar else 0) and built["fallbacks"] == 0 and (built["font_bytes"] > 0) == gvar
        # batching acts only together with gvar on the device: one call for the file's group, all its faces in it
        assert mgr.gvar_batch_stats() == ({"calls": 1, "faces": n} if gvar and batched else {"calls": 0, "faces": 0})
        # the stores stay: a second render uploads nothing and calls nothing
        assert _render(vg, mgr, renderer) == got and mgr.command_stats()["fonts_uploaded"] == 0
        assert mgr.gvar_batch_stats() == {"calls": 0, "faces": 0}


def test_preloading_builds_the_stores_of_a_group(vg, yardsticks):
    font, records = N.files()["shear"]
    r = vg.Renderer.new_precise(0)
    mgr = _manager(vg, commands=2, gvar=True, batched=True)
    mgr.add_font_named_instances(font)
    assert r.preload_fonts(mgr) > 0
    assert _render(vg, mgr, r) == yardsticks["shear"]
    assert mgr.command_stats()["fonts_uploaded"] == 0 and mgr.gvar_batch_stats() == {"calls": 0, "faces": 0}   # all there already


def test_instances_added_one_by_one_keep_their_own_calls(vg, renderer, yardsticks):
    font, records = N.files()["two_axes_no_room"]
    mgr = _manager(vg, commands=1, gvar=True, batched=True)
    for name, record in zip(N.instance_names(vg, font), records):
        mgr.add_font_instance(name, font, record["location"])
    assert _render(vg, mgr, renderer) == yardsticks["two_axes_no_room"]
    assert mgr.gvar_stats()["fonts_built"] == 3 and mgr.gvar_batch_stats() == {"calls": 0, "faces": 0}


def test_a_group_with_refused_positions(vg, renderer):
    """glyph ids whose variation data is malformed where their tuples are read: at two of the four positions the device refuses
    the face, those ids get their stores from the host reader, counted and remembered; the other two come from the batched call"""
    base = G.edge_faces()["composites_malformed"][0]
    records = [dict(subfamily="Bold", ps=None, location={"wght": 1.0}), dict(subfamily="Thin", ps=None, location={"wght": -0.5}),
               dict(subfamily="Regular", ps=None, location={"wght": 0.0}), dict(subfamily="Medium", ps=None, location={"wght": 0.5})]
    assert [all(G.restate(base, [int(r["location"]["wght"] * 16384)])["ok"]) for r in records] == [False, True, True, False]
    font = N.with_instances(base, records, room_for_ps=False)
    want = _one_instance_per_record(vg, renderer, font, records)
    assert len(want) >= 4
    for batched in (False, True):
        mgr = _manager(vg, commands=2, gvar=True, batched=batched)
        assert len(set(mgr.add_font_named_instances(font))) == 4
        assert _render(vg, mgr, renderer) == want
        assert mgr.gvar_stats()["fonts_built"] == 2 and mgr.gvar_stats()["fallbacks"] == 2
        assert mgr.command_stats()["fonts_uploaded"] == 4
        assert mgr.gvar_batch_stats() == ({"calls": 1, "faces": 4} if batched else {"calls": 0, "faces": 0})
        # the refusals are remembered, the host's stores stay: nothing is tried or counted again
        assert _render(vg, mgr, renderer) == want
        assert mgr.gvar_stats() == {"fonts_built": 0, "font_bytes": 0, "fallbacks": 0} and mgr.gvar_batch_stats() == {"calls": 0, "faces": 0}
