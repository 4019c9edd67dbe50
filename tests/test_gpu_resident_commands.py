"""Command fonts on the device, on real faces: outlines uploaded once as commands (vgsdf_font_create_commands), every glyph
rendered by (font, glyph id) (vgsdf_outlines_submit_resident).

The output contract is equality with the packed form of the commands the host's reader records for the same glyphs
(vgsdf_outlines_submit_packed) and, through the glyf fixture fonts, with the goldens: rects, sizes, every segment bit for bit,
every bitmap.  No tolerance appears anywhere.
"""
import hashlib

import numpy as np
import pytest

from test_golden_cpu import golden_rows
from test_gpu_resident_fonts import SETS, _assert_same
from conftest import noto_files
from fira_cff_kit import fira_cff_file, fira_cff_part_file  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _command_set(vg, mgr, fid):
    r = mgr.record_resident_commands(fid)
    descs = [mgr.command_font_desc(fid, k) for k in range(r["n_files"])]
    o = mgr.record_outlines(fid)
    packed = (o["cmd_off"],) + vg.SdfContext.pack_outlines(o["cmd_off"], o["cmds"])
    assert np.array_equal(o["ids"], r["ids"])
    return r, descs, packed


def _run_packed(ctx, packed, r, capacity):
    ctx.outlines_submit_packed(*packed, r["scale"], r["shift_x"], capacity=capacity)
    return ctx.outlines_wait(), ctx.outlines_segments(), None


def _run_by_name(ctx, fonts, r, capacity):
    ctx.outlines_submit_resident(fonts, r["font_of"], r["glyph_id"], r["scale"], r["shift_x"], capacity=capacity)
    return ctx.outlines_wait(), ctx.outlines_segments(), None


def _by_name_equals_packed(vg, mgr, fid):
    r, descs, packed = _command_set(vg, mgr, fid)
    n = len(r["ids"])
    ctx = vg.SdfContext(0)
    try:
        fonts = [ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"]) for d in descs]
        assert all(f.device_bytes >= 29 * len(d["kinds"]) + 4 * len(d["cmd_off"]) for f, d in zip(fonts, descs))
        want = _run_packed(ctx, packed, r, 8 << 20)
        cap = int(want[0][2]) + 64
        want = _run_packed(ctx, packed, r, cap)
        got = _run_by_name(ctx, fonts, r, cap)
        uploaded = ctx.resident_upload_bytes()
        _assert_same(got, want)
        # the same again (fonts stay resident, nothing about the first submission lingers)
        _assert_same(_run_by_name(ctx, fonts, r, cap), want)
        for f in fonts:
            f.free()
    finally:
        ctx.close()
    assert n > 1000 and uploaded <= 24 * n + 32 * len(descs) + 32      # 24 n + 4 without the PBF arrays, 32 per font
    return r, got


@pytest.mark.parametrize("which", list(SETS))
def test_all_glyphs_by_id_equal_the_packed_form_and_the_goldens(vg, which):
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name("Font", SETS[which] or noto_files())
    r, got = _by_name_equals_packed(vg, mgr, fid)
    (rects, bitmaps, _, _), _, _ = got
    raster = [row for row in golden_rows(which) if int(row["bitmap_size"])]
    has = np.flatnonzero(rects["has_raster"])
    assert len(raster) == len(has)
    at, bad = 0, []
    for gi, row in zip(has, raster):
        size = int(rects["w"][gi]) * int(rects["h"][gi])
        if int(row["codepoint"]) != int(r["ids"][gi]) or hashlib.sha256(bitmaps[at:at + size].tobytes()).hexdigest() != row["sha256"]:
            bad.append(row["codepoint"])
        at += size
    assert not bad and at == len(bitmaps), bad[:8]


def test_fira_as_cff_by_id_equals_its_packed_form(vg, fira_cff_file):
    mgr = vg.FontManager(True)
    fid = mgr.add_font_data("Fira CFF", fira_cff_file.read_bytes())
    with pytest.raises(RuntimeError, match="glyf"):      # no glyf-resident form: this is the face's only way by name
        mgr.record_resident(fid)
    r, got = _by_name_equals_packed(vg, mgr, fid)
    assert len(r["ids"]) == 1686 and int(got[0][0]["has_raster"].sum()) > 1500


# ---- the host façade with the switch on ----

def _pbf_shas(files):
    return {k.split("/", 1)[1].split("-")[0]: hashlib.sha256(v).hexdigest() for k, v in files.items()}


def _render(vg, mgr, r, *args):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r, *args)
    return w.files


NO_STATS = {"groups": 0, "fonts_uploaded": 0, "font_bytes": 0, "block_bytes": 0}


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place_pbf", "packed_bitmaps"])
@pytest.mark.parametrize("key", ["fira", "noto_regular", "noto_all"])
def test_facade_mode_2_writes_the_golden_files_from_command_stores(vg, key, in_place):
    import json
    from conftest import GOLDEN
    from test_golden_cpu import set_paths
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())[key]
    name, paths = set_paths(key)
    r = vg.Renderer.new_precise(0)
    mgr = vg.FontManager(True)
    mgr.set_resident_commands(2)
    mgr.set_in_place_pbf(in_place)
    mgr.add_font_with_name(name, paths)
    first = _render(vg, mgr, r)
    t1, s1, g1 = mgr.timings(), mgr.command_stats(), mgr.resident_stats()
    second = _render(vg, mgr, r)
    t2, s2 = mgr.timings(), mgr.command_stats()
    assert _pbf_shas(first) == golden and second == first
    # every group by name against command stores, the stores uploaded on the first render only
    assert s1["groups"] == t1["fe_groups"] >= 1 and t1["glyf_groups"] == 0 and t1["glyf_fallbacks"] == 0 and g1 == NO_STATS
    assert s1["fonts_uploaded"] == len(paths) and s1["font_bytes"] > 0
    assert s2["groups"] == t2["fe_groups"] == s1["groups"] and s2["fonts_uploaded"] == 0 and s2["font_bytes"] == 0
    assert 0 < s2["block_bytes"] <= 32 * t2["glyphs"] + 64 * len(paths) * s2["groups"] + 64 * s2["groups"]
    assert set(mgr.resident_stats()) == {"groups", "fonts_uploaded", "font_bytes", "block_bytes"}     # (its four fields, as ever)


def test_facade_mode_2_on_lanes_that_share_a_device_and_through_render_blocks(vg):
    import json
    from conftest import GOLDEN
    from test_golden_cpu import set_paths
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())
    name, paths = set_paths("noto_all")
    r = vg.Renderer.new_multi([0, 0])
    mgr = vg.FontManager(True)
    mgr.set_resident_commands(2)
    mgr.set_lane_form(2)
    fid = mgr.add_font_with_name(name, paths)
    files = _render(vg, mgr, r)
    s, t = mgr.command_stats(), mgr.timings()
    assert _pbf_shas(files) == golden["noto_all"]
    assert s["groups"] == t["fe_groups"] >= 2 and t["glyf_groups"] == 0 and t["glyf_fallbacks"] == 0
    assert s["fonts_uploaded"] == len(paths)          # one store per (device, face): the two lanes share them
    assert _render(vg, mgr, r) == files and mgr.command_stats()["font_bytes"] == 0
    # single blocks on demand (vg_manager_render_blocks)
    single = vg.Renderer.new_precise(0)
    one = vg.FontManager(True)
    one.set_resident_commands(2)
    fid = one.add_font_with_name(name, paths)
    for k, starts in enumerate(([0], [1024], [0x0900, 0x1000, 0])):
        w = vg.DummyWriter()
        one.render_glyphs(w, single, fid, starts)
        assert _pbf_shas(w.files) == {str(b): golden["noto_all"][str(b)] for b in starts}
        st = one.command_stats()
        assert st["groups"] >= 1 and (st["fonts_uploaded"] == len(paths)) == (k == 0)


def _two_font_managers(vg, fira_cff_file, fira_cff_part_file, mode):
    """one manager with Fira (glyf) and Fira-as-CFF as two font ids, one with both kinds of file under one font id (first
    provider wins: the CFF file draws the code points of its 400 glyphs, Fira Sans the others — blocks of both)"""
    from conftest import FIRA
    two = vg.FontManager(True)
    two.set_resident_commands(mode)
    two.add_font_with_name("Fira Glyf", [FIRA])
    two.add_font_with_name("Fira Cff", [fira_cff_file])
    one = vg.FontManager(True)
    one.set_resident_commands(mode)
    one.add_font_with_name("Fira Both", [fira_cff_part_file, FIRA])
    return two, one


@pytest.mark.parametrize("resident_fonts", [False, True], ids=["glyf_form", "resident_fonts"])
def test_facade_mode_1_sends_the_groups_without_a_glyf_form_by_name(vg, fira_cff_file, fira_cff_part_file, resident_fonts):
    r = vg.Renderer.new_precise(0)
    want = [_render(vg, m, r) for m in _two_font_managers(vg, fira_cff_file, fira_cff_part_file, 0)]
    for k, mgr in enumerate(_two_font_managers(vg, fira_cff_file, fira_cff_part_file, 1)):
        mgr.set_resident_fonts(resident_fonts)
        files = _render(vg, mgr, r)
        assert files == want[k]                                    # byte for byte the files of mode 0
        s, g, t = mgr.command_stats(), mgr.resident_stats(), mgr.timings()
        assert s["groups"] >= 1 and s["fonts_uploaded"] >= 1 and t["glyf_fallbacks"] == 0
        assert s["groups"] + g["groups"] + t["glyf_groups"] <= t["fe_groups"]
        assert _render(vg, mgr, r) == files and mgr.command_stats()["fonts_uploaded"] == 0
    # a manager of the glyf font alone: untouched by mode 1, its groups counted where they were
    from conftest import FIRA
    alone = vg.FontManager(True)
    alone.set_resident_commands(1)
    alone.set_resident_fonts(resident_fonts)
    alone.add_font_with_name("Fira Glyf", [FIRA])
    _render(vg, alone, r)
    t, g = alone.timings(), alone.resident_stats()
    assert alone.command_stats() == NO_STATS and (g["groups"] if resident_fonts else t["glyf_groups"]) == t["fe_groups"] >= 1


def test_budget_zero_keeps_todays_path(vg, fira_cff_file):
    files = {}
    for budget in (None, 0):
        r = vg.Renderer.new_precise(0)
        if budget is not None:
            r.set_resident_budget(budget)
        mgr = vg.FontManager(True)
        mgr.set_resident_commands(1)
        mgr.add_font_with_name("Fira Cff", [fira_cff_file])
        files[budget] = _render(vg, mgr, r)
        s = mgr.command_stats()
        if budget == 0:
            assert s == NO_STATS and mgr.timings()["fe_groups"] >= 1
        else:
            assert s["groups"] == mgr.timings()["fe_groups"] >= 1
    assert files[0] == files[None]


def test_preload_uploads_the_stores_the_mode_would_use(vg, fira_cff_file):
    """mode 1: the stores of the fonts that have no glyf form (a glyf font that comes to share a group with one gets its store on
    first use, as without preloading)"""
    r = vg.Renderer.new_precise(0)
    off = vg.FontManager(True)
    off.add_font_with_name("Fira Cff", [fira_cff_file])
    assert r.preload_fonts(off) == 0                       # mode 0: a CFF face has nothing to preload
    mgr = vg.FontManager(True)
    mgr.set_resident_commands(1)
    mgr.add_font_with_name("Fira Cff", [fira_cff_file])
    assert r.preload_fonts(mgr) > 0 and r.preload_fonts(mgr) == 0
    _render(vg, mgr, r)
    s = mgr.command_stats()
    assert s["groups"] >= 1 and s["fonts_uploaded"] == 0 and s["font_bytes"] == 0
