"""Variable `glyf` files rendered at chosen positions through the façade on the GPU (vg_manager_add_font_instance): a placed glyf
face is a command face, and every existing path takes it as one.

The independent yardstick is tests/gvar_instances_kit.py's yardstick_files: the points, component offsets and widths fontTools
has at the location, the reference's arithmetic in f64, the oracle's rings, precise raster and encoder — nothing of the product.
Every switch that changes who does the work (the device's glyf decoder and glyf stores — which must NOT take the face —, command
stores by glyph id or for every group, mixed stores beside a static glyf file, families, family tables built by the host or the
device with their HVAR part, in-place PBF, and the command store built by the host reader or by the device's gvar kernels) must
leave the bytes as they are, and the stats must say which stores were made and by whom."""
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
from conftest import FIRA  # noqa: E402

pytestmark = pytest.mark.gpu

NO_GLYF_WORK = {"built_on_device": 0, "bytes": 0, "fallbacks": 0}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def shear():
    return G.variable_glyf_fira("shear")


@pytest.fixture(scope="module")
def two_axes():
    return G.variable_glyf_fira("two_axes")


@pytest.fixture(scope="module")
def yardsticks(oracle, shear, two_axes):
    """computed once, shared, never changed"""
    return {"medium": G.yardstick_files(shear, {"wght": 650}, "synth_medium", oracle),
            "bold": G.yardstick_files(shear, {"wght": 900}, "synth_bold", oracle),
            "wide": G.yardstick_files(two_axes, G.EXACT_TWO_AXES[1], "synth_wide", oracle)}


def _manager(vg, glyf=False, commands=1, mixed=False, families=False, tables=False, in_place=True, gvar=False):
    mgr = vg.FontManager(True)
    mgr.set_gvar_on_device(gvar)
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


def test_instances_equal_the_independent_yardstick_with_every_switch_off(vg, renderer, shear, two_axes, yardsticks):
    mgr = vg.FontManager(True)
    assert mgr.add_font_instance("Synth Medium", shear, {"wght": 650}) == "synth_medium"
    assert mgr.add_font_instance("Synth Wide", two_axes, G.EXACT_TWO_AXES[1]) == "synth_wide"
    got = _render(vg, mgr, renderer)
    want = {**yardsticks["medium"], **yardsticks["wide"]}
    assert len(got) == len(want) == 512
    for path in want:
        assert got[path] == want[path], path
    # the position matters: the same file added plainly gives other bytes
    plain = vg.FontManager(True)
    plain.add_font_data("Synth Medium", shear)
    assert sum(a != b for a, b in zip(_render(vg, plain, renderer).values(), yardsticks["medium"].values())) >= 1


CONFIGS = [dict(commands=1), dict(commands=2), dict(glyf=True, commands=0), dict(glyf=True, commands=1), dict(glyf=True, commands=1, mixed=True),
           dict(commands=1, families=True), dict(commands=1, families=True, tables=True), dict(glyf=True, commands=2, families=True, tables=True),
           dict(glyf=True, commands=1, mixed=True, families=True, tables=True), dict(commands=1, in_place=False),
           dict(commands=2, families=True, tables=True, in_place=False)]


@pytest.mark.parametrize("gvar", [False, True], ids=["gvar_on_host", "gvar_on_device"])
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "_".join(f"{k}{int(v)}" for k, v in c.items()))
def test_the_files_do_not_depend_on_who_does_the_work(vg, renderer, shear, two_axes, yardsticks, config, gvar):
    for font, loc, name, key in ((shear, {"wght": 650}, "Synth Medium", "medium"), (two_axes, G.EXACT_TWO_AXES[1], "Synth Wide", "wide")):
        mgr = _manager(vg, gvar=gvar, **config)
        mgr.add_font_instance(name, font, loc)
        got = _render(vg, mgr, renderer)
        assert got == yardsticks[key], (name, config)
        # never a glyf form: no glyf store is built or uploaded, no group is decoded from glyf entries
        assert mgr.glyf_table_stats() == NO_GLYF_WORK and mgr.resident_stats()["fonts_uploaded"] == 0
        assert mgr.mixed_stats()["glyf_fonts"] == 0
        if config.get("commands"):
            assert mgr.command_stats()["fonts_uploaded"] == 1
            built = mgr.gvar_stats()
            assert built["fonts_built"] == int(gvar) and built["fallbacks"] == 0 and (built["font_bytes"] > 0) == gvar
        if config.get("families"):
            assert mgr.family_stats()["groups"] >= 1 and mgr.family_stats()["families_uploaded"] == 1
        assert mgr.family_table_stats() == {"built_on_device": int(bool(config.get("tables"))), "fallbacks": 0}


def test_an_instance_beside_a_static_glyf_file_in_mixed_stores(vg, renderer, shear, yardsticks):
    """two font ids in one manager, one a placed face (a command store), one a static glyf file (a glyf store): with mixed stores
    the group is submitted against both kinds, and each font id's files are what they are alone"""
    alone = vg.FontManager(True)
    alone.add_font_with_name("Fira Static", [FIRA])
    static = _render(vg, alone, renderer)
    for families in (False, True):
        mgr = _manager(vg, glyf=True, commands=1, mixed=True, families=families, tables=families)
        mgr.add_font_instance("Synth Medium", shear, {"wght": 650})
        mgr.add_font_with_name("Fira Static", [FIRA])
        got = _render(vg, mgr, renderer)
        assert got == {**yardsticks["medium"], **static}
        assert mgr.command_stats()["fonts_uploaded"] == 1 and mgr.resident_stats()["fonts_uploaded"] == 1
    # ... and under ONE name, the instance in front: its glyphs win, the static file fills in the rest from a glyf store
    mgr = _manager(vg, glyf=True, commands=1, mixed=True)
    mgr.add_font_instance("Synth Medium", shear, {"wght": 650})
    mgr.add_font_with_name("Synth Medium", [FIRA])
    both = _render(vg, mgr, renderer)
    stats = mgr.mixed_stats()
    assert stats["groups"] >= 1 and stats["glyf_fonts"] == 1 and stats["command_fonts"] == 1
    off = _manager(vg)
    off.add_font_instance("Synth Medium", shear, {"wght": 650})
    off.add_font_with_name("Synth Medium", [FIRA])
    assert both == _render(vg, off, renderer) and len(both) == 256


def test_a_face_the_device_refuses_goes_the_hosts_way_once_and_is_counted(vg, renderer):
    """a glyph id with malformed variation data: the device's builder refuses the face, the host reader's table makes the store"""
    font = G.edge_faces()["composites_malformed"][0]
    off = _manager(vg, commands=2)
    off.add_font_instance_normalized("Edge", font, [16384])
    want = _render(vg, off, renderer)
    assert off.gvar_stats() == {"fonts_built": 0, "font_bytes": 0, "fallbacks": 0}
    mgr = _manager(vg, commands=2, gvar=True)
    mgr.add_font_instance_normalized("Edge", font, [16384])
    assert _render(vg, mgr, renderer) == want and len(want) >= 1
    assert mgr.gvar_stats() == {"fonts_built": 0, "font_bytes": 0, "fallbacks": 1} and mgr.command_stats()["fonts_uploaded"] == 1
    # the refusal is remembered, the host's store stays: nothing is tried or counted again
    assert _render(vg, mgr, renderer) == want
    assert mgr.gvar_stats() == {"fonts_built": 0, "font_bytes": 0, "fallbacks": 0} and mgr.command_stats()["fonts_uploaded"] == 0
    # a good face beside it is built by the device
    good = _manager(vg, commands=2, gvar=True)
    good.add_font_instance_normalized("Edge", G.edge_faces()["inference"][0], [16384])
    host = _manager(vg, commands=2)
    host.add_font_instance_normalized("Edge", G.edge_faces()["inference"][0], [16384])
    assert _render(vg, good, renderer) == _render(vg, host, renderer)
    assert good.gvar_stats()["fonts_built"] == 1 and good.gvar_stats()["fallbacks"] == 0


@pytest.mark.parametrize("gvar", [False, True], ids=["gvar_on_host", "gvar_on_device"])
def test_two_instances_of_one_file_are_two_font_ids_with_two_stores(vg, renderer, shear, yardsticks, gvar):
    for config in (dict(commands=1, gvar=gvar), dict(glyf=True, commands=1, mixed=True, families=True, tables=True, gvar=gvar)):
        mgr = _manager(vg, **config)
        mgr.add_font_instance("Synth Medium", shear, {"wght": 650})
        mgr.add_font_instance("Synth Bold", shear, {"wght": 900})
        got = _render(vg, mgr, renderer)
        assert got == {**yardsticks["medium"], **yardsticks["bold"]}
        assert mgr.command_stats()["fonts_uploaded"] == 2 and mgr.gvar_stats()["fonts_built"] == 2 * int(gvar)
        if config.get("tables"):
            assert mgr.family_table_stats() == {"built_on_device": 2, "fallbacks": 0}
        # the stores stay: nothing is uploaded by the second render
        assert _render(vg, mgr, renderer) == got and mgr.command_stats()["fonts_uploaded"] == 0


def test_an_instance_at_the_default_position_is_the_file_added_plainly(vg, renderer, shear, two_axes):
    for font, loc in ((shear, {"wght": 400}), (two_axes, {})):
        for config in (dict(commands=1), dict(commands=1, families=True, tables=True)):
            a, b = _manager(vg, **config), _manager(vg, **config)
            a.add_font_instance("Same", font, loc)
            b.add_font_data("Same", font)
            assert _render(vg, a, renderer) == _render(vg, b, renderer)
