"""Family tables built on the device (vgsdf_family_create_tables) on the fixture fonts: whole Fira Sans and the 20-file Noto Sans
id are built both ways — from the host reader's table (vgsdf_family_create) and from the faces' cmap and hmtx tables — and read
back equal, for both kinds of store; and the host façade with vg_manager_set_family_tables_on_device writes the golden PBF files,
builds every family on the device, and falls back for a font id with an irregular cmap.  No tolerance appears anywhere."""
import json

import numpy as np
import pytest

import cmap_edge_tables as E
from conftest import FIRA, GOLDEN, noto_files
from test_golden_cpu import set_paths

pytestmark = pytest.mark.gpu

ARRAYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "cmd_pre", "leaf_pre", "pbf_fix")


@pytest.mark.parametrize("kind", ["commands", "glyf"])
@pytest.mark.parametrize("which", ["fira", "noto_all"])
def test_whole_fonts_are_built_both_ways_and_read_back_equal(vg, which, kind):
    paths = [FIRA] if which == "fira" else noto_files()
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name("Font", paths)
    t = mgr.family_desc(fid)
    descs = [mgr.family_tables_desc(fid, k) for k in range(len(paths))]
    ctx = vg.SdfContext(0)
    try:
        if kind == "glyf":
            fonts = [ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"]) for d in (mgr.resident_font_desc(fid, k) for k in range(len(paths)))]
        else:
            fonts = [ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"])
                     for d in (mgr.command_font_desc(fid, k) for k in range(len(paths)))]
        want = ctx.family_create(fonts, t["code_point"], t["font_of"], t["glyph_id"], t["advance"], t["scale"], t["shift_x"])
        got = ctx.family_create_tables(fonts, descs)
        a, b = ctx.family_read(got), ctx.family_read(want)
        for k in ARRAYS:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        n = len(t["code_point"])
        assert len(a["code_point"]) == n > 1000 and got.device_bytes == want.device_bytes and got.count(0, 0xFFFF) == n
        assert int(a["cmd_pre"][-1]) > n and (int(a["leaf_pre"][-1]) > 0) == (kind == "glyf")
        print(which, kind, "count / emit ms:", ctx.family_tables_kernel_ms())
        got.free(), want.free()
    finally:
        ctx.close()


def _manager(vg, mode, in_place):
    mgr = vg.FontManager(True)
    if mode == "fonts":
        mgr.set_resident_fonts(True)
    else:
        mgr.set_resident_commands(2)
    mgr.set_resident_families(True)
    mgr.set_family_tables_on_device(True)
    mgr.set_in_place_pbf(in_place)
    return mgr


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place_pbf", "packed_bitmaps"])
@pytest.mark.parametrize("mode", ["fonts", "commands"])
@pytest.mark.parametrize("key", ["fira", "noto_all"])
def test_facade_writes_the_golden_files_from_device_built_families(vg, key, mode, in_place):
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())[key]
    name, paths = set_paths(key)
    r = vg.Renderer.new_precise(0)
    mgr = _manager(vg, mode, in_place)
    mgr.add_font_with_name(name, paths)
    first = _render(vg, mgr, r)
    s1, f1, t1 = mgr.family_table_stats(), mgr.family_stats(), mgr.timings()
    assert _pbf_shas(first) == golden
    assert s1 == {"built_on_device": 1, "fallbacks": 0} and f1["families_uploaded"] == 1 and f1["groups"] == t1["fe_groups"] >= 1
    assert f1["family_bytes"] >= 27 * t1["glyphs"]
    assert _render(vg, mgr, r) == first and mgr.family_table_stats() == {"built_on_device": 0, "fallbacks": 0}
    # preloading builds the family the same way: the first render of another manager on the renderer is warm
    other = _manager(vg, mode, in_place)
    other.add_font_with_name(name, paths)
    assert r.preload_fonts(other) > 0 and r.preload_fonts(other) == 0          # (another manager: other faces, other tables)
    assert _render(vg, other, r) == first and other.family_stats()["families_uploaded"] == 0


def test_facade_falls_back_for_a_font_id_with_an_irregular_cmap(vg):
    from test_family_tables_desc_host import splice
    from test_gpu_resident_fonts import _render
    # Fira Sans with its own tables but for one overlapping pair of format 12 groups in front of them
    face = dict(E.irregular_cases()["format12_overlap"])
    import struct
    from fontTools import ttLib
    ttf = ttLib.TTFont(str(FIRA), lazy=True)
    cmap = ttf.reader["cmap"]
    n = struct.unpack_from(">H", cmap, 2)[0]
    recs = [struct.unpack_from(">HHI", cmap, 4 + 8 * i) for i in range(n)]
    body = cmap[4 + 8 * n:]
    extra = E.fmt12([(0x41, 0x45, 36), (0x45, 0x46, 40)])
    head = b"".join(struct.pack(">HHI", p, e, o + 8) for p, e, o in recs) + struct.pack(">HHI", 3, 10, 4 + 8 * (n + 1) + len(body))
    face.update(cmap=struct.pack(">HH", 0, n + 1) + head + body + extra, hmtx=ttf.reader["hmtx"], units_per_em=ttf["head"].unitsPerEm,
                num_glyphs=ttf["maxp"].numGlyphs, num_hmetrics=ttf["hhea"].numberOfHMetrics)
    data = splice(face)
    r = vg.Renderer.new_precise(0)
    files = {}
    for way in ("device", "host"):
        mgr = _manager(vg, "fonts", True)
        mgr.set_family_tables_on_device(way == "device")
        fid = mgr.add_font_data("Irregular", data)
        if way == "device":
            assert mgr.family_tables_desc(fid, 0) is None
        files[way] = _render(vg, mgr, r)
        stats = mgr.family_table_stats()
        assert stats == ({"built_on_device": 0, "fallbacks": 1} if way == "device" else {"built_on_device": 0, "fallbacks": 0})
        assert mgr.family_stats()["groups"] >= 1
    assert files["device"] == files["host"] and len(files["device"]) == 256
