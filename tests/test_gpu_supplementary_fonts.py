"""The façade with vg_manager_set_supplementary_planes on, over the 20-file Noto Sans id, on every route: host tessellation,
the device front-end's packed and glyf-parts forms, glyphs named against resident fonts and against command stores, resident
families (one family per plane of the font id, the tasks with the low halves), mixed stores, and family tables on the device; packed
bitmaps and in-place PBF.  vg_manager_render_blocks writes the five supplementary blocks (U+10700, U+11100, U+11300, U+1DF00,
U+1E700: 140 code points) and the BMP blocks 0 and 0x0900; every supplementary file equals the oracle's — Font.render_glyph per
code point, first provider wins, oracle.pbf_encode (tests/supplementary_planes_kit.py) — and the BMP files are what the switch-off
run writes and what tests/golden/pbf_sha256.json holds.  A whole run writes 261 files, on one lane and on two lanes of one device
in every lane form.  With union outlines on the run completes and the pass has seen the 140 glyphs (no byte comparison: those
bitmaps are not the reference's by design).  Every comparison is byte for byte."""
import hashlib
import json

import pytest

import supplementary_planes_kit as S
from conftest import GOLDEN, noto_files

pytestmark = pytest.mark.gpu

BMP = (0, 0x0900)
STARTS = list(S.NOTO_BLOCKS) + list(BMP)
# route -> (device front-end, glyf on device, resident fonts, resident commands, families, mixed stores, tables on device)
ROUTES = {
    "host_tessellation": (False, False, False, 0, False, False, False),
    "packed": (True, False, False, 0, False, False, False),
    "glyf_parts": (True, True, False, 0, False, False, False),
    "resident_named": (True, True, True, 0, False, False, False),
    "commands_named": (True, True, False, 2, False, False, False),
    "resident_families": (True, True, True, 0, True, False, False),
    "command_families": (True, True, False, 2, True, False, False),
    "mixed_stores": (True, True, True, 1, True, True, False),
    "family_tables_on_device": (True, True, True, 0, True, False, True),
}


def _manager(vg, route, on=True, in_place=True):
    fe, glyf, fonts, commands, families, mixed, tables = ROUTES[route]
    m = vg.FontManager(True)
    m.set_device_front_end(fe)
    m.set_glyf_on_device(glyf)
    m.set_resident_fonts(fonts)
    m.set_resident_commands(commands)
    m.set_resident_families(families)
    m.set_mixed_stores(mixed)
    m.set_family_tables_on_device(tables)
    m.set_in_place_pbf(in_place)
    m.set_supplementary_planes(on)
    return m, m.add_font_with_name("Noto Sans Regular", noto_files())


def _name(fid, start):
    return f"{fid}/{start}-{start + 255}.pbf"


def _blocks(vg, m, r, fid, starts):
    w = vg.DummyWriter()
    m.render_glyphs(w, r, fid, starts)
    return w.files


@pytest.fixture(scope="module")
def renderer(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's five files, computed once"""
    fonts = S.OracleFonts(oracle, noto_files())
    assert tuple(fonts.blocks()) == S.NOTO_BLOCKS
    return {start: fonts.block_pbf("noto_sans_regular", start, oracle.PRECISE) for start in S.NOTO_BLOCKS}


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "pbf_sha256.json").read_text())["noto_all"]


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place_pbf", "packed_bitmaps"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_writes_the_oracles_files(vg, renderer, want, golden, route, in_place):
    m, fid = _manager(vg, route, True, in_place)
    assert fid == "noto_sans_regular" and tuple(m.supplementary_blocks(fid)) == S.NOTO_BLOCKS
    files = _blocks(vg, m, renderer, fid, STARTS)
    assert sorted(files) == sorted(_name(fid, s) for s in STARTS)
    for start in S.NOTO_BLOCKS:
        assert files[_name(fid, start)] == want[start], hex(start)
    off, _ = _manager(vg, route, False, in_place)
    before = _blocks(vg, off, renderer, fid, list(BMP))
    for start in BMP:
        assert files[_name(fid, start)] == before[_name(fid, start)]
        assert hashlib.sha256(before[_name(fid, start)]).hexdigest() == golden[str(start)]
    with pytest.raises(RuntimeError, match="bad block start"):
        _blocks(vg, off, renderer, fid, [0x10700])
    if route in ("resident_families", "command_families", "family_tables_on_device"):
        # every group went as ranges, the supplementary blocks against the font id's family of plane 1
        f, t = m.family_stats(), m.timings()
        assert f["groups"] == t["fe_groups"] >= 1 and f["families_uploaded"] == 2
        assert m.resident_stats()["groups"] == 0 and m.command_stats()["groups"] == 0
        if route == "family_tables_on_device":
            # both planes built by the device (vgsdf_family_create_tables_at for plane 1), the planes chosen by ONE census call
            assert m.family_table_stats() == {"built_on_device": 2, "fallbacks": 0}
            assert m.family_plane_stats() == {"census_calls": 1, "built_on_device": 1, "stated_by_host": 0, "planes": 2}
            again = _blocks(vg, m, renderer, fid, STARTS)              # warm: nothing is built, nothing is counted again
            assert again == files and m.family_plane_stats() == {"census_calls": 0, "built_on_device": 0, "stated_by_host": 0, "planes": 0}
        else:
            assert m.family_table_stats() == {"built_on_device": 0, "fallbacks": 0}
            assert m.family_plane_stats() == {"census_calls": 0, "built_on_device": 0, "stated_by_host": 1, "planes": 2}
    assert m.render_block(renderer, fid, 0x1E700) == want[0x1E700]


def test_a_whole_run_with_the_switch_off_is_the_golden_run(vg, renderer, golden):
    m, fid = _manager(vg, "resident_families", False)
    w = vg.DummyWriter()
    m.render_glyphs(w, renderer)
    assert len(w.files) == 256
    assert {str(int(k.split("/")[1].split("-")[0])): hashlib.sha256(v).hexdigest() for k, v in w.files.items()} == golden


@pytest.mark.parametrize("form", [2, 1, 0])
@pytest.mark.parametrize("route", ["packed", "resident_families"])
def test_a_whole_run_on_one_and_on_two_lanes(vg, renderer, want, golden, route, form):
    """261 files: the 256 of the golden run and the oracle's five; two lanes of one device write the same in every lane form (a
    supplementary block goes whole to lane (start / 256) % 2)"""
    m, fid = _manager(vg, route)
    w = vg.DummyWriter()
    m.render_glyphs(w, renderer)
    one = w.files
    assert len(one) == 261
    for start in S.NOTO_BLOCKS:
        assert one[_name(fid, start)] == want[start]
    for start, sha in golden.items():
        assert hashlib.sha256(one[_name(fid, int(start))]).hexdigest() == sha
    two = vg.Renderer.new_multi([0, 0])
    try:
        m2, _ = _manager(vg, route)
        m2.set_lane_form(form)
        w2 = vg.DummyWriter()
        m2.render_glyphs(w2, two)
        assert w2.files == one
        assert m2.reduced_counters()[0] == 261
    finally:
        two.close()


@pytest.mark.parametrize("route", ["host_tessellation", "glyf_parts"])
def test_union_outlines_see_the_supplementary_glyphs(vg, renderer, route):
    m, fid = _manager(vg, route)
    m.set_union_outlines(True)
    files = _blocks(vg, m, renderer, fid, list(S.NOTO_BLOCKS))
    assert len(files) == 5 and all(len(v) > 0 for v in files.values())
    stats = m.union_stats()
    assert stats["seen"] == S.NOTO_CODE_POINTS, stats


def _with_plane_1(font_bytes):
    """the font with one more cmap subtable, format 12 over U+10400 .. U+10403 -> glyph ids 36 .. 39"""
    import io
    import struct
    from fontTools import ttLib
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    import cmap_edge_tables as E
    ttf = ttLib.TTFont(io.BytesIO(font_bytes), lazy=True)
    cmap = ttf.reader["cmap"]
    n = struct.unpack_from(">H", cmap, 2)[0]
    recs = [struct.unpack_from(">HHI", cmap, 4 + 8 * i) for i in range(n)]
    body = cmap[4 + 8 * n:]
    head = b"".join(struct.pack(">HHI", p, e, o + 8) for p, e, o in recs) + struct.pack(">HHI", 3, 10, 4 + 8 * (n + 1) + len(body))
    t = DefaultTable("cmap")
    t.data = struct.pack(">HH", 0, n + 1) + head + body + E.fmt12([(0x10400, 0x10403, 36)])
    ttf["cmap"] = t
    out = io.BytesIO()
    ttf.save(out)
    return out.getvalue()


def test_a_placed_face_takes_the_hosts_table_for_its_supplementary_plane(vg, renderer):
    """an fvar instance (glyf + gvar) with four code points in plane 1: with family tables on the device its plane-0 family is
    built by the device, its plane-1 family is stated by the host (vgsdf_family_create_at) and counted as such, no census is
    taken; the files are those of the same manager without families"""
    import gvar_instances_kit as G
    font = _with_plane_1(G.variable_glyf_fira("shear"))
    files = {}
    for families in (False, True):
        m = vg.FontManager(True)
        m.set_resident_commands(2)
        m.set_resident_families(families)
        m.set_family_tables_on_device(families)
        m.set_supplementary_planes(True)
        fid = m.add_font_instance("Synth Medium", font, {"wght": 650})
        assert m.supplementary_blocks(fid) == {0x10400: 4}
        files[families] = _blocks(vg, m, renderer, fid, [0x10400, 0])
        if families:
            assert m.family_stats()["groups"] == m.timings()["fe_groups"] >= 1 and m.family_stats()["families_uploaded"] == 2
            assert m.family_plane_stats() == {"census_calls": 0, "built_on_device": 0, "stated_by_host": 1, "planes": 2}
            assert m.family_table_stats() == {"built_on_device": 1, "fallbacks": 0}
    assert files[True] == files[False] and len(files[True]) == 2 and len(files[True][_name(fid, 0x10400)]) > 100
