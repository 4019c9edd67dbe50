"""Variable CFF2 files rendered at chosen positions through the façade on the GPU (vg_manager_add_font_instance).

The independent yardstick is tests/variable_instances_kit.py's yardstick_files: fontTools' outlines and widths at the location,
the reference's arithmetic in f64, the oracle's rings, precise raster and encoder — nothing of the product.  Every switch that
changes who does the work (command stores by glyph id or for every group, charstrings decoded by the host or the device,
families, family tables built by the host or the device, in-place PBF) must leave the bytes as they are, and the stats must show
that the device did the work where it was switched on."""
import pytest

pytest.importorskip("fontTools")

import variable_instances_kit as K  # noqa: E402

pytestmark = pytest.mark.gpu

NO_CHARSTRINGS = {"fonts_decoded": 0, "font_bytes": 0, "fallbacks": 0}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def fira1():
    return K.variable_fira(120)


@pytest.fixture(scope="module")
def fira2():
    return K.variable_fira(120, two_axes=True)


@pytest.fixture(scope="module")
def yardsticks(oracle, fira1, fira2):
    """computed once, shared, never changed"""
    return {"medium": K.yardstick_files(fira1, {"wght": 650}, "synth_medium", oracle),
            "bold": K.yardstick_files(fira1, {"wght": 900}, "synth_bold", oracle),
            "wide": K.yardstick_files(fira2, K.EXACT_TWO_AXES, "synth_wide", oracle)}


def _manager(vg, commands=1, charstrings=0, families=False, tables=False, in_place=True):
    mgr = vg.FontManager(True)
    mgr.set_resident_commands(commands)
    mgr.set_charstrings_on_device(charstrings)
    mgr.set_resident_families(families)
    mgr.set_family_tables_on_device(tables)
    mgr.set_in_place_pbf(in_place)
    return mgr


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


def test_instances_equal_the_independent_yardstick_with_every_switch_off(vg, renderer, fira1, fira2, yardsticks):
    mgr = vg.FontManager(True)
    assert mgr.add_font_instance("Synth Medium", fira1, {"wght": 650}) == "synth_medium"
    assert mgr.add_font_instance("Synth Wide", fira2, K.EXACT_TWO_AXES) == "synth_wide"
    got = _render(vg, mgr, renderer)
    want = {**yardsticks["medium"], **yardsticks["wide"]}
    assert len(got) == len(want) == 512
    for path in want:
        assert got[path] == want[path], path
    # the position matters: the same file added plainly gives other bytes
    plain = vg.FontManager(True)
    plain.add_font_data("Synth Medium", fira1)
    assert sum(a != b for a, b in zip(_render(vg, plain, renderer).values(), yardsticks["medium"].values())) >= 1


CONFIGS = [dict(commands=1), dict(commands=2), dict(commands=1, charstrings=2), dict(commands=2, charstrings=2),
           dict(commands=1, families=True), dict(commands=1, charstrings=2, families=True),
           dict(commands=1, families=True, tables=True), dict(commands=2, charstrings=2, families=True, tables=True),
           dict(commands=1, charstrings=2, families=True, tables=True, in_place=False), dict(commands=1, in_place=False),
           dict(commands=2, families=True, tables=True, in_place=False)]


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "_".join(f"{k}{int(v)}" for k, v in c.items()))
def test_the_files_do_not_depend_on_who_does_the_work(vg, renderer, fira1, fira2, yardsticks, config):
    for font, loc, name, key in ((fira1, {"wght": 650}, "Synth Medium", "medium"), (fira2, K.EXACT_TWO_AXES, "Synth Wide", "wide")):
        mgr = _manager(vg, **config)
        mgr.add_font_instance(name, font, loc)
        got = _render(vg, mgr, renderer)
        assert got == yardsticks[key], (name, config)
        cs, ft = mgr.charstring_stats(), mgr.family_table_stats()
        assert mgr.command_stats()["fonts_uploaded"] == 1
        if config.get("charstrings") == 2:
            assert cs["fonts_decoded"] == 1 and cs["fallbacks"] == 0
        else:
            assert cs == NO_CHARSTRINGS
        if config.get("families"):
            assert mgr.family_stats()["groups"] >= 1 and mgr.family_stats()["families_uploaded"] == 1
        if config.get("tables"):
            assert ft == {"built_on_device": 1, "fallbacks": 0}
        else:
            assert ft == {"built_on_device": 0, "fallbacks": 0}


def test_two_instances_of_one_file_are_two_font_ids_with_two_stores(vg, renderer, fira1, yardsticks):
    for config in (dict(commands=1), dict(commands=1, charstrings=2, families=True, tables=True)):
        mgr = _manager(vg, **config)
        mgr.add_font_instance("Synth Medium", fira1, {"wght": 650})
        mgr.add_font_instance("Synth Bold", fira1, {"wght": 900})
        got = _render(vg, mgr, renderer)
        assert got == {**yardsticks["medium"], **yardsticks["bold"]}
        assert mgr.command_stats()["fonts_uploaded"] == 2
        if config.get("tables"):
            assert mgr.family_table_stats() == {"built_on_device": 2, "fallbacks": 0} and mgr.charstring_stats()["fonts_decoded"] == 2
        # the stores stay: nothing is uploaded by the second render
        assert _render(vg, mgr, renderer) == got and mgr.command_stats()["fonts_uploaded"] == 0


def test_an_hvar_the_description_refuses_goes_the_hosts_way_once(vg, renderer):
    font, refused, desc_refused = K.hvar_edge_faces()["map_format2"]
    assert desc_refused and not refused
    files = {}
    for tables in (False, True):
        mgr = _manager(vg, commands=1, families=True, tables=tables)
        mgr.add_font_instance_normalized("Edge", font, [8192])
        files[tables] = _render(vg, mgr, renderer)
        assert mgr.family_table_stats() == {"built_on_device": 0, "fallbacks": int(tables)}
        if tables:   # remembered: no second attempt, no second fallback
            assert _render(vg, mgr, renderer) == files[tables] and mgr.family_table_stats() == {"built_on_device": 0, "fallbacks": 0}
    assert files[True] == files[False] and len(files[True]) == 256
    # ... and a neighbour whose HVAR the device takes gives, on the device, what the host gives
    font = K.hvar_edge_faces()["map1_size3_bits16"][0]
    for coords in K.EDGE_POSITIONS:
        both = {}
        for tables in (False, True):
            mgr = _manager(vg, commands=1, families=True, tables=tables)
            mgr.add_font_instance_normalized("Edge", font, coords)
            both[tables] = _render(vg, mgr, renderer)
            assert mgr.family_table_stats() == {"built_on_device": int(tables), "fallbacks": 0}
        assert both[True] == both[False]


def test_an_instance_at_the_default_position_is_the_file_added_plainly(vg, renderer, fira1, fira2):
    for font, loc in ((fira1, {"wght": 400}), (fira2, {})):
        for config in (dict(commands=1), dict(commands=1, charstrings=2, families=True, tables=True)):
            a, b = _manager(vg, **config), _manager(vg, **config)
            a.add_font_instance("Same", font, loc)
            b.add_font_data("Same", font)
            assert _render(vg, a, renderer) == _render(vg, b, renderer)
