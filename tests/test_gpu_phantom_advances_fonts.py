"""Placed `glyf` files WITHOUT `HVAR` through the façade on the GPU with vg_manager_set_gvar_advances: the 315-glyph fixtures of
tests/phantom_advances_kit.py at wght 650, where every advance differs from `hmtx`.

The independent yardstick is the kit's yardstick_files: fontTools' points and the widths it has after drawing a glyph (the
phantom points'), the reference's arithmetic in f64, the oracle's rings, precise raster and encoder.  Who does the work — glyphs
named one by one or code-point ranges of resident families, the family's table from the host reader or built by the device with
the phantom pass, the command store from the reader or from the device's gvar kernels — must leave the bytes as they are, and the
stats must say who did it."""
import pytest

pytest.importorskip("fontTools")

import phantom_advances_kit as P  # noqa: E402

pytestmark = pytest.mark.gpu

LOCATION = {"wght": 650}


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def yardsticks(oracle):
    """computed once, shared, never changed"""
    return {kind: P.yardstick_files(P.without_hvar(kind), LOCATION, "synth_medium", oracle) for kind in ("shear", "two_axes")}


def _manager(vg, on=True, commands=1, families=False, tables=False, gvar=False, in_place=True):
    mgr = vg.FontManager(True)
    mgr.set_gvar_advances(on)
    mgr.set_gvar_on_device(gvar)
    mgr.set_resident_commands(commands)
    mgr.set_resident_families(families)
    mgr.set_family_tables_on_device(tables)
    mgr.set_in_place_pbf(in_place)
    return mgr


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


CONFIGS = [dict(commands=1), dict(commands=1, families=True), dict(commands=1, families=True, tables=True),
           dict(commands=1, families=True, tables=True, gvar=True), dict(commands=2, families=True, tables=True, gvar=True, in_place=False)]


@pytest.mark.parametrize("kind", ["shear", "two_axes"])
def test_the_switch_off_run_keeps_hmtx_and_differs(vg, renderer, yardsticks, kind):
    off = _manager(vg, on=False)
    assert off.add_font_instance("Synth Medium", P.without_hvar(kind), LOCATION) == "synth_medium"
    got = _render(vg, off, renderer)
    assert set(got) == set(yardsticks[kind]) and sum(got[p] != yardsticks[kind][p] for p in got) >= 2
    assert off.gvar_advance_stats() == {"faces": 0, "device_builds": 0, "fallbacks": 0}


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "_".join(f"{k}{int(v)}" for k, v in c.items()))
@pytest.mark.parametrize("kind", ["shear", "two_axes"])
def test_the_files_equal_the_yardstick_whoever_does_the_work(vg, renderer, yardsticks, kind, config):
    mgr = _manager(vg, **config)
    mgr.add_font_instance("Synth Medium", P.without_hvar(kind), LOCATION)
    got = _render(vg, mgr, renderer)
    assert got == yardsticks[kind], config
    tables = int(bool(config.get("tables")))
    assert mgr.gvar_advance_stats() == {"faces": 1, "device_builds": tables, "fallbacks": 0}
    assert mgr.family_table_stats() == {"built_on_device": tables, "fallbacks": 0}
    if config.get("families"):
        assert mgr.family_stats()["groups"] >= 1 and mgr.family_stats()["families_uploaded"] == 1
    built = mgr.gvar_stats()
    assert built["fonts_built"] == int(bool(config.get("gvar"))) and built["fallbacks"] == 0


def test_a_face_the_device_refuses_falls_back_and_is_counted(vg, renderer):
    """a glyph id past VGSDF_GVAR_MAX_DELTAS: the phantom pass refuses the face by the count, the host reader's table makes the family"""
    font = P.over_budget_face()
    host = _manager(vg, families=True)
    host.add_font_instance_normalized("Edge", font, [16384])
    want = _render(vg, host, renderer)
    assert host.gvar_advance_stats() == {"faces": 1, "device_builds": 0, "fallbacks": 0} and len(want) >= 1
    mgr = _manager(vg, families=True, tables=True)
    mgr.add_font_instance_normalized("Edge", font, [16384])
    assert _render(vg, mgr, renderer) == want
    assert mgr.gvar_advance_stats() == {"faces": 1, "device_builds": 0, "fallbacks": 1}
    assert mgr.family_table_stats() == {"built_on_device": 0, "fallbacks": 1}
    # the advances did move (glyph id 0 takes a delta), and a good face beside it is built by the device
    off = _manager(vg, on=False, families=True)
    off.add_font_instance_normalized("Edge", font, [16384])
    assert _render(vg, off, renderer) != want
    good = _manager(vg, families=True, tables=True)
    good.add_font_instance_normalized("Edge", P.faces()["point_lists"][0], [16384])
    ref = _manager(vg, families=True)
    ref.add_font_instance_normalized("Edge", P.faces()["point_lists"][0], [16384])
    assert _render(vg, good, renderer) == _render(vg, ref, renderer)
    assert good.gvar_advance_stats() == {"faces": 1, "device_builds": 1, "fallbacks": 0}
