"""The device's builder of a placed `glyf` face's command store (vgsdf_font_create_gvar) on the 315-glyph fixtures of
tests/gvar_instances_kit.py — (a) the sheared master, every delta explicit; (b) the pure-scale master, most points inferred, the
values not exact in f32; (c) two axes, intermediate regions and shared tuples — at three positions each: the device's store
equals, byte for byte, the store vgsdf_font_create_commands makes of the host reader's command table, and occupies as much."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402

pytestmark = pytest.mark.gpu

POSITIONS = {"shear": [{"wght": 525}, {"wght": 650}, {"wght": 900}], "scale": [{"wght": 525}, {"wght": 700}, {"wght": 900}],
             "two_axes": G.EXACT_TWO_AXES[:2] + [{"wght": 700, "wdth": 130}]}


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", ["shear", "scale", "two_axes"])
def test_the_device_store_is_the_host_store(vg, ctx, kind):
    font = G.variable_glyf_fira(kind)
    stores = set()
    for loc in POSITIONS[kind]:
        mgr = vg.FontManager(False)
        fid = mgr.add_font_instance("Synth", font, loc)
        desc, host = mgr.gvar_font_desc(fid), mgr.command_font_desc(fid)
        assert desc["num_glyphs"] == 315 and len(host["kinds"]) > 8000
        a = ctx.font_create_gvar(desc)
        b = ctx.font_create_commands(host["cmd_off"], host["dat_off"], host["kinds"], host["coords"])
        try:
            ra, rb = ctx.font_commands_read(a), ctx.font_commands_read(b)
            assert np.array_equal(ra["cmd_off"], rb["cmd_off"]) and np.array_equal(rb["cmd_off"], host["cmd_off"])
            assert ra["records"].tobytes() == rb["records"].tobytes()
            assert ra["context"].tobytes() == rb["context"].tobytes()
            assert a.device_bytes == b.device_bytes
            stores.add(ra["records"].tobytes())
        finally:
            a.free()
            b.free()
    assert len(stores) == 3          # the position matters
