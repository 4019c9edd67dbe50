"""Glyf fonts of several faces built by one call (vgsdf_fonts_create_tables) on the fixture fonts: the 20 Noto Sans files and Fira
Sans go through ONE call and each comes back equal to vgsdf_font_create of its restated arrays (tests/composite_edge_trees.py,
pinned to the host reader on the CPU); and the host façade with vg_manager_set_glyf_tables_batched writes the golden PBF files
from fonts a font id's files got in one call, counts them as it counts the fonts of the per-face call, shares them between two
lanes of a device, and falls back for a refused face without losing its neighbour.  No tolerance appears anywhere."""
import json

import pytest

import composite_edge_trees as T
from conftest import FIRA, GOLDEN, noto_files
from test_golden_cpu import set_paths

pytestmark = pytest.mark.gpu


def test_fixture_fonts_in_one_call_read_back_equal(vg):
    ctx = vg.SdfContext(0)
    mgr = vg.FontManager(False)
    paths = noto_files() + [FIRA]
    assert len(paths) == 21
    descs = []
    for p in paths:
        descs.append(mgr.font_tables_desc(mgr.add_font_with_name(p.stem, [p]), 0))
    res = ctx.fonts_create_tables(descs)
    print("count / emit ms of the one call:", ctx.fonts_tables_kernel_ms())
    assert len(res) == len(paths)
    for p, d, (got, status, _) in zip(paths, descs, res):
        assert status == 0 and got is not None, p.stem
        t = T.Tables(d["loca"], d["glyf"], d["num_glyphs"], d["loca_entries"], d["loca_long"])
        r = T.restate(t)
        want = ctx.font_create(r["leaf_off"], r["leaves"], r["bytes"])
        a, b = ctx.font_read(got), ctx.font_read(want)
        for k in ("leaf_off", "leaves", "bytes"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (p.stem, k)
            assert a[k].tobytes() == r[k].tobytes(), (p.stem, k)
        assert got.device_bytes == want.device_bytes and len(a["leaves"]) >= t.num_glyphs // 2, p.stem
        got.free(), want.free()
    ctx.close()


def _manager(vg, families, batched=True):
    mgr = vg.FontManager(True)
    mgr.set_resident_fonts(True)
    if families:
        mgr.set_resident_families(True)
        mgr.set_family_tables_on_device(True)
    mgr.set_glyf_tables_on_device(True)
    mgr.set_glyf_tables_batched(batched)
    return mgr


@pytest.mark.parametrize("families", [False, True], ids=["glyph_named_groups", "families_with_tables_on_device"])
@pytest.mark.parametrize("key", ["fira", "noto_all"])
def test_facade_writes_the_golden_files_from_fonts_built_in_one_call(vg, key, families):
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
    assert mgr.glyf_table_batch_stats() == {"calls": 1, "faces": len(paths)}
    assert t1["glyf_groups"] == 0 and t1["glyf_fallbacks"] == 0
    if families:
        assert mgr.family_table_stats() == {"built_on_device": 1, "fallbacks": 0} and mgr.family_stats()["groups"] == t1["fe_groups"] >= 1
    else:
        assert r1["groups"] == t1["fe_groups"] >= 1
    assert _render(vg, mgr, r) == first and mgr.glyf_table_stats() == {"built_on_device": 0, "bytes": 0, "fallbacks": 0}
    assert mgr.glyf_table_batch_stats() == {"calls": 0, "faces": 0}
    # preloading builds the fonts the same way: the first render of another manager on the renderer is warm
    other = _manager(vg, families)
    other.add_font_with_name(name, paths)
    assert r.preload_fonts(other) > 0 and r.preload_fonts(other) == 0
    assert _render(vg, other, r) == first and other.glyf_table_stats()["built_on_device"] == 0 and other.resident_stats()["fonts_uploaded"] == 0
    assert other.glyf_table_batch_stats() == {"calls": 0, "faces": 0}


def test_the_switch_alone_changes_nothing(vg):
    """without vg_manager_set_glyf_tables_on_device the batched switch has no effect: the host's tables, no call"""
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())["fira"]
    name, paths = set_paths("fira")
    mgr = vg.FontManager(True)
    mgr.set_resident_fonts(True)
    mgr.set_glyf_tables_batched(True)
    mgr.add_font_with_name(name, paths)
    assert _pbf_shas(_render(vg, mgr, vg.Renderer.new_precise(0))) == golden
    assert mgr.glyf_table_stats()["built_on_device"] == 0 and mgr.glyf_table_batch_stats() == {"calls": 0, "faces": 0}
    assert mgr.resident_stats()["fonts_uploaded"] == 1


def test_facade_two_lanes_build_each_face_once(vg):
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
    assert mgr.glyf_table_batch_stats() == {"calls": 1, "faces": len(paths)}   # the lane that came second found them all
    assert _render(vg, mgr, r) == files and mgr.glyf_table_stats()["built_on_device"] == 0


def test_facade_a_refused_face_between_good_ones(vg):
    """a font id whose one face is past the slot bound, beside Fira Sans: the files are those of the switch off, one fallback,
    counted once, and Fira Sans is still built on the device (the shape of test_facade_falls_back_for_a_font_past_the_bounds);
    then the refused face BETWEEN two copies of Fira Sans in one font id, so that all three go through one call"""
    from test_gpu_resident_fonts import _render
    data = T.font_of(T.slots_font(1024))
    r = vg.Renderer.new_precise(0)

    def manager(way, one_block=False):
        mgr = vg.FontManager(True)
        mgr.set_resident_fonts(True)
        mgr.set_glyf_tables_on_device(way == "batched")
        mgr.set_glyf_tables_batched(way == "batched")
        if one_block:
            mgr.set_threads(0, 1)                 # one block per submission: Fira's groups hold no other font
        return mgr

    files = {}
    for way in ("batched", "host"):
        mgr = manager(way)
        mgr.add_font_data("Fan Out", data)
        mgr.add_font_with_name("Fira Sans Regular", [FIRA])
        files[way] = _render(vg, mgr, r)
        assert mgr.glyf_table_stats()["fallbacks"] == (1 if way == "batched" else 0)
        if way == "batched":
            assert _render(vg, mgr, r) == files[way] and mgr.glyf_table_stats()["fallbacks"] == 0     # remembered per face and device
    assert files["batched"] == files["host"] and len(files["batched"]) >= 2
    mgr = manager("batched", one_block=True)
    mgr.add_font_data("Fan Out", data)
    mgr.add_font_with_name("Fira Sans Regular", [FIRA])
    assert _render(vg, mgr, r) == files["host"] and mgr.glyf_table_stats()["built_on_device"] == 1
    # one font id, three faces, one call: the refused face costs its neighbours nothing
    both = {}
    for way in ("batched", "host"):
        mgr = manager(way)
        mgr.add_font_with_name("Mixed", [FIRA])
        mgr.add_font_data("Mixed", data)
        mgr.add_font_with_name("Mixed", [FIRA])
        both[way] = _render(vg, mgr, r)
        if way == "batched":
            assert mgr.glyf_table_stats()["fallbacks"] == 1 and mgr.glyf_table_stats()["built_on_device"] == 2
            assert mgr.glyf_table_batch_stats() == {"calls": 1, "faces": 3}
            assert _render(vg, mgr, r) == both[way]
            assert mgr.glyf_table_stats() == {"built_on_device": 0, "bytes": 0, "fallbacks": 0} and mgr.glyf_table_batch_stats() == {"calls": 0, "faces": 0}
    assert both["batched"] == both["host"] and len(both["batched"]) >= 2
