"""The three younger device decoders under random input: charstring_decode for `CFF ` and for CFF2 (vgsdf_font_create_charstrings,
vgsdf_font_create_charstrings2) and the gvar builders (vgsdf_font_create_gvar, vgsdf_fonts_create_gvar, vgsdf_gvar_advance_deltas)
on the faces of tests/charstring_fuzz_kit.py and tests/gvar_fuzz_kit.py, which tests/test_decoder_fuzz_host.py holds against the
host reader, the kits' interpreters and fontTools on the CPU.

The comparison is the one of the regimes tests: the store the device builds and the store vgsdf_font_create_commands makes of the
host reader's table are read back (vgsdf_font_commands_read) and must be equal in cmd_off, records, context bytes and device_bytes.
A CFF2 face is also decoded with two arrays of blend factors no position produces, against the kit's interpreter (the host reader
has no such position).  One face per decoder is rendered by glyph id (vgsdf_outlines_submit_resident) against the oracle's raster
of the kit's callbacks.  Glyph counts: 192 and 128 (three and two full waves), 65 and 63.  Every program was run to its end by
the kit's interpreter within its token cap when the face was made."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring2_edge_programs as K2  # noqa: E402
import charstring_fuzz_kit as F  # noqa: E402
import gvar_fuzz_kit as GF  # noqa: E402
import gvar_instances_kit as G  # noqa: E402

pytestmark = pytest.mark.gpu

# (seed, glyph ids): eight faces of three (charstrings) or two (gvar) full waves, one of 65 and one of 63
CHARSTRING_FACES = [(s, F.N_GLYPHS) for s in F.SEEDS] + [(9, 65), (10, 63)]
GVAR_FACES = [(s, GF.N_GLYPHS) for s in GF.SEEDS] + [(9, 65), (10, 63)]
SCALE = 24.0 / 2048


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def _store(ctx, font):
    r = ctx.font_commands_read(font)
    return r["cmd_off"].tobytes(), r["records"].tobytes(), r["context"].tobytes(), font.device_bytes


def assert_store_is(ctx, built, table):
    """the device-built font against the store of a command table; frees both"""
    want = ctx.font_create_commands(table["cmd_off"], table["dat_off"], table["kinds"], table["coords"])
    try:
        a, b = _store(ctx, built), _store(ctx, want)
        assert np.array_equal(np.frombuffer(b[0], np.uint32), table["cmd_off"])
        for got, expected, what in zip(a, b, ("cmd_off", "records", "context", "device_bytes")):
            assert got == expected, what
    finally:
        built.free()
        want.free()


@pytest.mark.parametrize("seed, n", CHARSTRING_FACES)
def test_cff_faces_decode_to_the_host_readers_store(vg, ctx, seed, n):
    desc, host = F.host_views(vg, F.face(seed, False, n).font(), False)
    assert len(host["cmd_off"]) == n + 1 and len(host["kinds"]) > 5 * n
    assert_store_is(ctx, ctx.font_create_charstrings(desc), host)


@pytest.mark.parametrize("seed, n", CHARSTRING_FACES)
def test_cff2_faces_decode_to_the_host_readers_store_and_follow_other_factors(vg, ctx, seed, n):
    desc, host = F.host_views(vg, F.face(seed, True, n).font(), True)
    assert len(host["cmd_off"]) == n + 1 and len(host["kinds"]) > 5 * n
    assert_store_is(ctx, ctx.font_create_charstrings2(desc), host)
    for shift in (0, 3):
        d = dict(desc, **K2.alt_sets(desc, shift))
        want, _ = K2.expected_commands(d, budget=F.MAX_RUN_TOKENS)
        assert want["coords"].tobytes() != host["coords"].tobytes()
        assert_store_is(ctx, ctx.font_create_charstrings2(d), want)


@pytest.mark.parametrize("seed, n", GVAR_FACES)
def test_gvar_faces_build_the_host_readers_store_alone_and_batched(vg, ctx, seed, n):
    f = GF.face(seed, n)
    views = [GF.host_views(vg, f, c) for c in f.positions]
    singles = []
    for desc, host, _ in views:
        assert len(host["cmd_off"]) == n + 1
        font = ctx.font_create_gvar(desc)
        singles.append(_store(ctx, font))
        assert_store_is(ctx, font, host)
    fonts, status, _ = ctx.fonts_create_gvar(views[0][0], f.positions)
    try:
        assert list(status) == [0] * len(f.positions) and all(font is not None for font in fonts)
        for font, single in zip(fonts, singles):
            assert _store(ctx, font) == single
    finally:
        for font in fonts:
            if font is not None:
                font.free()


@pytest.mark.parametrize("seed, n", GVAR_FACES)
def test_gvar_advance_deltas_are_the_host_readers(vg, ctx, seed, n):
    """(no face of the kit has an HVAR: rule G7 holds for all of them)"""
    f = GF.face(seed, n)
    moved = 0
    for coords in f.positions:
        desc, _, (want_d, want_state) = GF.host_views(vg, f, coords)
        got_d, got_state = ctx.gvar_advance_deltas(desc)
        assert got_state.tolist() == want_state.tolist()
        assert G.bits(got_d) == G.bits(want_d)
        moved += int(np.count_nonzero(got_d))
    assert moved > 0


def _callbacks(table, g):
    """glyph id g of a command table as the oracle's ring builder takes them: (kind, x1, y1, x2, y2, x, y)"""
    out, at = [], int(table["dat_off"][g])
    for kind in table["kinds"][table["cmd_off"][g]:table["cmd_off"][g + 1]]:
        n = {G.M: 2, G.L: 2, G.Q: 4, G.C: 6, G.Z: 0}[int(kind)]
        c = [float(v) for v in table["coords"][at:at + n]]
        at += n
        out.append((int(kind),) + tuple({0: [0.0] * 6, 2: [0.0] * 4 + c, 4: c[:2] + [0.0, 0.0] + c[2:], 6: c}[n]))
    return out


def assert_rendered_like_the_oracle(oracle, ctx, font, table, limit=48):
    """the glyph ids of the device-built `font` that deliver commands, by glyph id, against the oracle's rings and raster of the
    callbacks of `table` (the kit's)"""
    counts = np.diff(table["cmd_off"].astype(np.int64))
    gids = np.flatnonzero(counts > 0)[:limit]
    n = len(gids)
    ctx.outlines_submit_resident([font], np.zeros(n, np.uint16), gids, np.full(n, SCALE), np.zeros(n), capacity=8 << 20)
    rects, bitmaps, out_bytes, _ = ctx.outlines_wait()
    assert bitmaps is not None
    at = checked = 0
    for i, g in enumerate(gids):
        segs = []
        for ring in oracle.build_rings(_callbacks(table, int(g))):
            p = ring * SCALE
            segs.append(np.concatenate([p[:-1], p[1:]], axis=1))
        r = rects[i]
        if not r["has_raster"]:
            assert not segs, int(g)
            continue
        size = int(r["w"]) * int(r["h"])
        want = oracle.sdf_render(np.concatenate(segs), int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]))
        assert np.array_equal(bitmaps[at:at + size].reshape(want.shape), want), int(g)
        at += size
        checked += 1
    assert at == out_bytes and checked >= limit // 2


def test_a_face_of_each_decoder_renders_like_the_oracles_raster_of_the_kits_callbacks(oracle, vg, ctx):
    import charstring_edge_programs as K
    for cff2 in (False, True):
        desc, _ = F.host_views(vg, F.face(1, cff2).font(), cff2)
        kit, _ = (K2 if cff2 else K).expected_commands(desc, budget=F.MAX_RUN_TOKENS)
        font = (ctx.font_create_charstrings2 if cff2 else ctx.font_create_charstrings)(desc)
        try:
            assert_rendered_like_the_oracle(oracle, ctx, font, kit)
        finally:
            font.free()
    f = GF.face(1)
    desc, _, _ = GF.host_views(vg, f, f.positions[0])
    font = ctx.font_create_gvar(desc)
    try:
        assert_rendered_like_the_oracle(oracle, ctx, font, G.restate(f.font, f.positions[0]))
    finally:
        font.free()
