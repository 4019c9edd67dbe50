"""The three 315-glyph variable fixtures of tests/gvar_instances_kit.py (Fira Sans' outlines under one axis with explicit deltas,
one axis with inferred deltas, two axes with intermediate regions and shared tuples) at their three exact positions each, built
by ONE device call (vgsdf_fonts_create_gvar): every font equals, byte for byte, the store vgsdf_font_create_commands makes of the
host reader's command table at that position, and the one the single call makes there."""
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def _store(ctx, font):
    r = ctx.font_commands_read(font)
    return r["cmd_off"].tobytes(), r["records"].tobytes(), r["context"].tobytes(), font.device_bytes


@pytest.mark.parametrize("kind", ["shear", "scale", "two_axes"])
def test_a_fixture_at_its_exact_positions_in_one_call(vg, ctx, kind):
    font = G.variable_glyf_fira(kind)
    described = []
    for i, location in enumerate(G.EXACT_TWO_AXES if kind == "two_axes" else G.EXACT_ONE_AXIS):
        mgr = vg.FontManager(False)
        fid = mgr.add_font_instance(f"Synth {i}", font, location)
        described.append((mgr.gvar_font_desc(fid), mgr.command_font_desc(fid)))
    positions = [desc["coords"] for desc, _ in described]
    fonts, status, needed = ctx.fonts_create_gvar(described[0][0], positions)
    made = []
    try:
        assert status == [0, 0, 0] and needed == [0, 0, 0] and all(f is not None for f in fonts)
        stores = [_store(ctx, f) for f in fonts]
        assert len(set(stores)) == 3                     # three positions, three different stores
        for p, (desc, host) in enumerate(described):
            assert len(host["cmd_off"]) == 316
            made = [ctx.font_create_commands(host["cmd_off"], host["dat_off"], host["kinds"], host["coords"]), ctx.font_create_gvar(desc)]
            assert stores[p] == _store(ctx, made[0]), (kind, p)
            assert stores[p] == _store(ctx, made[1]), (kind, p)
            for f in made:
                f.free()
            made = []
        ms = ctx.fonts_gvar_kernel_ms()
        assert all(v > 0 for v in ms)
    finally:
        for f in list(fonts) + made:
            if f is not None:
                f.free()
