"""Glyf fonts built on the device (vgsdf_font_create_tables) on the fixture fonts: Fira Sans and each of the 20 Noto Sans files are
built both ways — vgsdf_font_create of the restated arrays (tests/composite_edge_trees.py, pinned to the host reader on the CPU)
and the device's walk over the face's own loca and glyf — and read back equal; and the host façade with
vg_manager_set_glyf_tables_on_device writes the golden PBF files, builds every font on the device, and falls back for a font past
the bounds of the resident form.  No tolerance appears anywhere."""
import json

import pytest

import composite_edge_trees as T
from conftest import FIRA, GOLDEN, noto_files
from test_golden_cpu import set_paths

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


@pytest.mark.parametrize("path", [FIRA] + noto_files(), ids=lambda p: p.stem)
def test_fixture_fonts_are_built_both_ways_and_read_back_equal(vg, ctx, path):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("One", [path])
    d = mgr.font_tables_desc(fid, 0)
    t = T.Tables(d["loca"], d["glyf"], d["num_glyphs"], d["loca_entries"], d["loca_long"])
    r = T.restate(t)
    want = ctx.font_create(r["leaf_off"], r["leaves"], r["bytes"])
    got = ctx.font_create_tables(d)
    a, b = ctx.font_read(got), ctx.font_read(want)
    for k in ("leaf_off", "leaves", "bytes"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert a[k].tobytes() == r[k].tobytes(), k
    assert got.device_bytes == want.device_bytes and len(a["leaves"]) >= t.num_glyphs // 2
    print(path.stem, t.num_glyphs, "glyph ids,", len(a["leaves"]), "leaves; count / emit ms:", ctx.font_tables_kernel_ms())
    got.free(), want.free()


def _manager(vg, families):
    mgr = vg.FontManager(True)
    mgr.set_resident_fonts(True)
    if families:
        mgr.set_resident_families(True)
        mgr.set_family_tables_on_device(True)
    mgr.set_glyf_tables_on_device(True)
    return mgr


@pytest.mark.parametrize("families", [False, True], ids=["glyph_named_groups", "families_with_tables_on_device"])
@pytest.mark.parametrize("key", ["fira", "noto_all"])
def test_facade_writes_the_golden_files_from_device_built_fonts(vg, key, families):
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())[key]
    name, paths = set_paths(key)
    r = vg.Renderer.new_precise(0)
    mgr = _manager(vg, families)
    mgr.add_font_with_name(name, paths)
    first = _render(vg, mgr, r)
    s1, r1, t1 = mgr.glyf_table_stats(), mgr.resident_stats(), mgr.timings()
    assert _pbf_shas(first) == golden
    assert s1["built_on_device"] == len(paths) == r1["fonts_uploaded"] and s1["fallbacks"] == 0 and s1["bytes"] == r1["font_bytes"] > 0
    assert t1["glyf_groups"] == 0 and t1["glyf_fallbacks"] == 0
    if families:
        assert mgr.family_table_stats() == {"built_on_device": 1, "fallbacks": 0} and mgr.family_stats()["groups"] == t1["fe_groups"] >= 1
    else:
        assert r1["groups"] == t1["fe_groups"] >= 1
    assert _render(vg, mgr, r) == first and mgr.glyf_table_stats() == {"built_on_device": 0, "bytes": 0, "fallbacks": 0}
    # preloading builds the fonts the same way: the first render of another manager on the renderer is warm
    other = _manager(vg, families)
    other.add_font_with_name(name, paths)
    assert r.preload_fonts(other) > 0 and r.preload_fonts(other) == 0
    assert _render(vg, other, r) == first and other.glyf_table_stats()["built_on_device"] == 0 and other.resident_stats()["fonts_uploaded"] == 0


def test_facade_two_lanes_share_the_device_built_fonts(vg):
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())["noto_all"]
    name, paths = set_paths("noto_all")
    r = vg.Renderer.new_multi([0, 0])
    mgr = _manager(vg, False)
    mgr.add_font_with_name(name, paths)
    files = _render(vg, mgr, r)
    s = mgr.glyf_table_stats()
    assert _pbf_shas(files) == golden
    assert s["built_on_device"] == len(paths) and s["fallbacks"] == 0          # one per (device, face): the lanes share them
    assert _render(vg, mgr, r) == files and mgr.glyf_table_stats()["built_on_device"] == 0


@pytest.mark.parametrize("bound", ["slots", "leaves"])
def test_facade_falls_back_for_a_font_past_the_bounds(vg, bound):
    """1024 leaves of 65537 command slots in one glyph id, or one leaf more than 2^22 in the face (its code points kept for the two
    smallest composites only: the face is refused whole, what is rendered is small): the device refuses the face, the host's table
    is not ok either, and the font's groups go the way they go with the switch off — one fallback counted, once"""
    from test_gpu_resident_fonts import _render
    data = T.font_of(T.slots_font(1024)) if bound == "slots" else T.font_of(T.leaves_font(1), mapped={1, 2})
    r = vg.Renderer.new_precise(0)
    files = {}
    for way in ("device", "host"):
        mgr = vg.FontManager(True)
        mgr.set_resident_fonts(True)
        mgr.set_glyf_tables_on_device(way == "device")
        mgr.add_font_data("Fan Out", data)
        mgr.add_font_with_name("Fira Sans Regular", [FIRA])
        files[way] = _render(vg, mgr, r)
        s = mgr.glyf_table_stats()
        assert s["fallbacks"] == (1 if way == "device" else 0)
        if way == "device":
            assert _render(vg, mgr, r) == files[way] and mgr.glyf_table_stats()["fallbacks"] == 0     # remembered per face and device
    assert files["device"] == files["host"] and len(files["device"]) >= 2
    # beside it under another font id's groups, Fira Sans is built on the device as ever
    mgr = vg.FontManager(True)
    mgr.set_resident_fonts(True)
    mgr.set_glyf_tables_on_device(True)
    mgr.set_threads(0, 1)                         # one block per submission: Fira's groups hold no other font
    mgr.add_font_data("Fan Out", data)
    mgr.add_font_with_name("Fira Sans Regular", [FIRA])
    both = _render(vg, mgr, r)
    assert both == files["host"] and mgr.glyf_table_stats()["built_on_device"] == 1
