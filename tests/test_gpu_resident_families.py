"""Resident families through the C ABI (vgsdf_family_create, vgsdf_outlines_submit_ranges) on real fonts, and what the two
entry points refuse.

A family is built from the table the host records for a font id (vg_manager_record_resident: code point -> file, glyph id,
advance, scale, shift_x).  Every 256-code-point block of the font as one task of ONE submission must equal the resident form of
the same glyph sequence — rects, every segment bit for bit, every bitmap, the PBF positions (tests/test_gpu_resident_fonts.py's
_assert_same) — and the golden SHAs.  No tolerance appears anywhere.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import family_ranges_kit as K
from test_golden_cpu import golden_rows
from test_gpu_resident_fonts import _assert_same, _font_set, _upload

pytestmark = pytest.mark.gpu

E_ARG = -1


def _family_of(ctx, fonts, r):
    assert (np.diff(r["ids"].astype(np.int64)) > 0).all() and int(r["ids"][-1]) <= 0xFFFF
    return ctx.family_create(fonts, r["ids"], r["font_of"], r["glyph_id"], r["advances"], r["scale"], r["shift_x"])


@pytest.mark.parametrize("which", ["fira", "noto_all"])
def test_every_block_as_one_submission_equals_the_resident_form_and_the_goldens(vg, which):
    _, _, _, r, descs = _font_set(vg, which)
    n = len(r["ids"])
    blocks = sorted(set((r["ids"] // 256).tolist()))
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        fam = _family_of(ctx, fonts, r)
        assert fam.count(0, 0xFFFF) == n and fam.device_bytes >= 27 * n
        first, last = np.array(blocks) * 256, np.array(blocks) * 256 + 255
        pre = 20 + np.arange(len(blocks)) % 7
        fix = K.fix_of(r["ids"], r["advances"])
        per_glyph_pre = np.zeros(n, np.uint32)
        per_glyph_pre[np.searchsorted(r["ids"], first)] = pre
        for pbf in (False, True):
            kw = dict(pbf_pre=per_glyph_pre, pbf_fix=fix) if pbf else {}
            ctx.outlines_submit_resident(fonts, r["font_of"], r["glyph_id"], r["scale"], r["shift_x"], capacity=64 << 20, **kw)
            want = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf else None)
            ctx.outlines_submit_ranges([fam], np.zeros(len(blocks), int), first, last, capacity=64 << 20, pbf_pre=pre if pbf else None)
            got = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf else None)
            _assert_same(got, want)
            assert ctx.resident_upload_bytes() == 32 * (len(blocks) + 1 + len(fonts))       # nothing per glyph
            if pbf:
                begin = ctx.outlines_task_extents()
                assert len(begin) == len(blocks) + 1 and begin[0] == 0 and int(begin[-1]) == got[0][2] and (np.diff(begin.astype(np.int64)) > 0).all()
            else:
                packed = got
        fam.free()
    finally:
        ctx.close()
    (rects, bitmaps, _, _), _, _ = packed
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


@pytest.fixture()
def kits(vg):
    ctx = vg.SdfContext(0)
    try:
        yield K.command_kit(vg, ctx), K.glyf_kit(vg, ctx)
    finally:
        ctx.close()


def test_bad_submissions_are_refused_and_the_context_goes_on(vg, kits):
    cmd, glyf = kits
    ctx = cmd.ctx
    a = K.random_family(cmd, 1, 200)
    g = K.random_family(glyf, 2, 200)

    def refused(families, tasks, **kw):
        fo, first, last, room = [np.array([t[i] for t in tasks], np.int64) for i in range(4)]
        with pytest.raises(vg.VgsdfError) as e:
            ctx.outlines_submit_ranges([f.handle for f in families], fo, first, last, capacity=1 << 20, pbf_pre=room, **kw)
        assert e.value.code == E_ARG
        # a submission after a refused one, on the same context
        K.compare(ctx, [a], [(0, int(a.cp[3]), int(a.cp[40]), 12)], layouts=(True,))

    whole = (0, 0, 0xFFFF, 5)
    refused([a, g], [whole])                                         # families of both kinds, named or not
    refused([g, a], [whole, (1, 0, 100, 0)])
    refused([a], [whole, (0, 50, 49, 0)])                            # first > last
    refused([a], [whole, (1, 0, 100, 0)])                            # family_of past n_families
    refused([], [whole])
    many = K.Family(cmd, [0] * 40000, a.cp, a.font_of, a.gid, a.advance, a.scale, a.shift)
    refused([many, many], [whole])                                   # 80000 fonts over the families
    K.compare(ctx, [many], [(0, int(a.cp[0]), int(a.cp[30]), 3)], layouts=(True,))      # (40000 are fine)
    # more than 2^31 - 1 command slots: 60000 entries of the 5000-command glyph, named eight times over
    n = 60000
    huge = K.Family(cmd, [0], np.arange(n), np.zeros(n, int), np.full(n, cmd.big), np.zeros(n), np.full(n, 0.024), np.zeros(n))
    refused([huge], [whole] * 8)
    # NULL arrays, NULL description
    L = vg.load_library()
    from versatiles_glyphs_rs_amd.device import _COutlinesRanges
    fams = (C.c_void_p * 1)(a.handle._h)
    one = np.zeros(1, np.uint16)
    for null in ("families", "family_of", "first", "last"):
        co = _COutlinesRanges(1, 1, C.cast(fams, C.c_void_p), one.ctypes.data, one.ctypes.data, one.ctypes.data)
        setattr(co, null, None)
        assert L.vgsdf_outlines_submit_ranges(ctx._h, C.byref(co), None, 0) == E_ARG
    assert L.vgsdf_outlines_submit_ranges(ctx._h, None, None, 0) == E_ARG
    K.compare(ctx, [a], [(0, 0, 0xFFFF, 7)])
    K.compare(glyf.ctx, [g], [(0, 0, 0xFFFF, 7)])                     # either kind alone renders


def test_bad_descriptions_are_refused_and_the_context_goes_on(vg, kits):
    cmd, glyf = kits
    ctx = cmd.ctx
    a = K.random_family(cmd, 3, 100)
    n_ids = 23    # glyph ids of a synthetic command font (test_gpu_resident_gather_regimes.LENGTHS)

    def refused(fonts, **change):
        args = dict(code_point=a.cp, font_of=a.font_of, glyph_id=a.gid, advance=a.advance, scale=a.scale, shift_x=a.shift)
        args.update(change)
        with pytest.raises(vg.VgsdfError) as e:
            ctx.family_create(fonts, **args)
        assert e.value.code == E_ARG
        K.compare(ctx, [a], [(0, int(a.cp[5]), int(a.cp[60]), 9)], layouts=(True,))

    fonts = [cmd.kinds[0]]
    bad = a.cp.copy()
    bad[10], bad[11] = bad[11], bad[10]
    refused(fonts, code_point=bad)                                   # not ascending
    bad = a.cp.copy()
    bad[11] = bad[10]
    refused(fonts, code_point=bad)                                   # ... not strictly
    bad = a.font_of.copy()
    bad[7] = 1
    refused(fonts, font_of=bad)                                      # font_of past n_fonts
    bad = a.gid.copy()
    bad[99] = n_ids
    refused(fonts, glyph_id=bad)                                     # a glyph id past its face
    refused([cmd.kinds[0], glyf.kinds[0]])                           # fonts of both kinds
    refused([])                                                      # no font
    L = vg.load_library()
    h = C.c_void_p()
    assert L.vgsdf_family_create(ctx._h, None, C.byref(h)) == E_ARG and not h.value
    # a family without an entry maps nothing
    none = K.Family(cmd, [0], [], [], [], [], [], [])
    assert none.handle.count(0, 0xFFFF) == 0
    assert len(K.compare(ctx, [none, a], [(0, 0, 0xFFFF, 4), (1, int(a.cp[0]), int(a.cp[9]), 5), (0, 3, 9, 6)])) == 10


def test_a_family_is_shared_by_the_contexts_of_its_device(vg, kits):
    cmd, _ = kits
    a = K.random_family(cmd, 4, 300)
    other = vg.SdfContext(0)
    try:
        tasks = [(0, int(a.cp[0]), int(a.cp[149]), 0), (0, int(a.cp[150]), int(a.cp[299]), 0)]
        want = K.compare(cmd.ctx, [a], tasks, layouts=(False,))
        # created through one context, named by two, both in flight at once
        cmd.ctx.outlines_submit_ranges([a.handle], [0], [tasks[0][1]], [tasks[0][2]], capacity=K.CAPACITY)
        other.outlines_submit_ranges([a.handle], [0], [tasks[1][1]], [tasks[1][2]], capacity=K.CAPACITY)
        ra, rb = cmd.ctx.outlines_wait(), other.outlines_wait()
        assert np.array_equal(np.concatenate([ra[0], rb[0]]), want)
    finally:
        other.close()


# ---- the host façade with vg_manager_set_resident_families on ----

def _golden(key):
    import json
    from conftest import GOLDEN
    from test_golden_cpu import set_paths
    return json.loads((GOLDEN / "pbf_sha256.json").read_text())[key], set_paths(key)


def _families_on(vg, mode):
    """mode: "fonts" = resident glyf fonts, "commands" = command-store mode 2"""
    mgr = vg.FontManager(True)
    if mode == "fonts":
        mgr.set_resident_fonts(True)
    else:
        mgr.set_resident_commands(2)
    mgr.set_resident_families(True)
    return mgr


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place_pbf", "packed_bitmaps"])
@pytest.mark.parametrize("mode", ["fonts", "commands"])
@pytest.mark.parametrize("key", ["fira", "noto_all"])
def test_facade_writes_the_golden_files_from_families(vg, key, mode, in_place):
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden, (name, paths) = _golden(key)
    r = vg.Renderer.new_precise(0)
    mgr = _families_on(vg, mode)
    mgr.set_in_place_pbf(in_place)
    fid = mgr.add_font_with_name(name, paths)
    first = _render(vg, mgr, r)
    t1, f1 = mgr.timings(), mgr.family_stats()
    second = _render(vg, mgr, r)
    t2, f2 = mgr.timings(), mgr.family_stats()
    assert _pbf_shas(first) == golden and second == first
    # every group went as ranges: none by glyph names, none through the glyf form or the reader
    assert f1["groups"] == t1["fe_groups"] >= 1 and t1["glyf_groups"] == 0 and t1["glyf_fallbacks"] == 0
    assert mgr.resident_stats()["groups"] == 0 and mgr.command_stats()["groups"] == 0
    assert f1["families_uploaded"] == 1 and f1["family_bytes"] >= 27 * t1["glyphs"]
    assert f2["groups"] == f1["groups"] and f2["families_uploaded"] == 0 and f2["family_bytes"] == 0
    # the block holds 32 bytes per task that maps a glyph, family and font: nothing per glyph
    n_busy = len(set((mgr.family_desc(fid)["code_point"] // 256).tolist()))      # blocks that map a glyph: one task each
    assert f2["block_bytes"] == 32 * (n_busy + (1 + len(paths)) * f2["groups"])
    # preloading builds the fonts and the family: the first render of another manager on the renderer is warm
    other = _families_on(vg, mode)
    other.add_font_with_name(name, paths)
    assert r.preload_fonts(other) > 0 and r.preload_fonts(other) == 0
    assert _render(vg, other, r) == first and other.family_stats()["families_uploaded"] == 0


def _planned_tasks(mgr, fid, world):
    """(tasks, (block, lane) pairs of more than one task, blocks that map a glyph) of the hybrid plan on `world` lanes: a block
    one lane holds whole is one task, a block split between lanes one task per lane and run of mapped code points it keeps"""
    owner, n_split, _ = mgr.plan_lanes(fid, world)
    tasks = multi = busy = 0
    for b in range(256):
        o = owner[256 * b:256 * b + 256]
        lanes = set(o[o != 0xFF].tolist())
        busy += bool(lanes)
        if len(lanes) == 1:
            tasks += 1
        for lane in lanes if len(lanes) > 1 else ():
            own = (o == lane).astype(np.int8)
            runs = int(own[0]) + int(np.count_nonzero(np.diff(own) == 1))
            tasks += runs
            multi += runs > 1
    return tasks, multi, busy, n_split


@pytest.mark.parametrize("mode", ["fonts", "commands"])
def test_facade_two_lanes_share_the_device(vg, mode):
    """{0, 0}: two lanes on one device share the font id's family; at two lanes the hybrid plan keeps every block of this
    font whole (the split is the next test's)"""
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden, (name, paths) = _golden("noto_all")
    r = vg.Renderer.new_multi([0, 0])
    mgr = _families_on(vg, mode)
    mgr.set_lane_form(2)
    fid = mgr.add_font_with_name(name, paths)
    files = _render(vg, mgr, r)
    f, t = mgr.family_stats(), mgr.timings()
    assert _pbf_shas(files) == golden
    assert f["groups"] == t["fe_groups"] >= 2 and t["glyf_groups"] == 0 and t["glyf_fallbacks"] == 0
    assert f["families_uploaded"] == 1                       # one per (device, font id): the lanes share it
    tasks, _, busy, n_split = _planned_tasks(mgr, fid, 2)
    assert n_split == 0 and tasks == busy and f["block_bytes"] == 32 * (tasks + (1 + len(paths)) * f["groups"])
    assert _render(vg, mgr, r) == files and mgr.family_stats()["families_uploaded"] == 0


@pytest.mark.parametrize("mode", ["fonts", "commands"])
def test_facade_the_hybrid_plan_splits_blocks_into_runs_of_code_points(vg, mode):
    """eight lanes on one device: the plan splits the heaviest blocks of Fira Sans between lanes, and such a block goes, in
    every lane that holds a part of it, as one task per run of code points the lane keeps.  The split is asserted, not assumed:
    the plan says so, some lane holds more than one run of a block, and the upload blocks hold exactly that many tasks"""
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden, (name, paths) = _golden("fira")
    r = vg.Renderer.new_multi([0] * 8)
    try:
        mgr = _families_on(vg, mode)
        mgr.set_lane_form(2)
        fid = mgr.add_font_with_name(name, paths)
        tasks, multi, busy, n_split = _planned_tasks(mgr, fid, 8)
        assert n_split >= 1 and multi >= 1 and tasks > busy
        files = _render(vg, mgr, r)
        f, t = mgr.family_stats(), mgr.timings()
        assert _pbf_shas(files) == golden
        assert f["groups"] == t["fe_groups"] >= 2 and t["glyf_groups"] == 0 and t["glyf_fallbacks"] == 0
        assert mgr.resident_stats()["groups"] == 0 and mgr.command_stats()["groups"] == 0
        # 32 bytes per task, and per group its one family and its one font: more tasks went than there are busy blocks
        n_tasks = f["block_bytes"] // 32 - 2 * f["groups"]
        assert f["block_bytes"] % 32 == 0 and n_tasks > busy, (f, busy, tasks)
        assert _render(vg, mgr, r) == files and mgr.family_stats()["families_uploaded"] == 0
    finally:
        r.close()


def test_facade_glyph_sharding_keeps_todays_path(vg):
    from test_gpu_resident_fonts import _pbf_shas, _render
    golden, (name, paths) = _golden("fira")
    r = vg.Renderer.new_multi([0, 0])
    mgr = _families_on(vg, "fonts")
    mgr.set_lane_form(0)                                     # glyph-level shards of every font
    mgr.add_font_with_name(name, paths)
    files = _render(vg, mgr, r)
    assert _pbf_shas(files) == golden
    assert mgr.family_stats() == {"groups": 0, "families_uploaded": 0, "family_bytes": 0, "block_bytes": 0}
    assert mgr.resident_stats()["groups"] >= 1


def test_facade_a_family_is_rebuilt_when_a_file_is_added(vg):
    from conftest import FIRA, NOTO
    from test_gpu_resident_fonts import _render
    r = vg.Renderer.new_precise(0)
    mgr = _families_on(vg, "fonts")
    fid = mgr.add_font_with_name("Two", [FIRA])
    _render(vg, mgr, r)
    assert mgr.family_stats()["families_uploaded"] == 1
    mgr.add_font_with_name("Two", [NOTO])
    with_families = _render(vg, mgr, r)
    assert mgr.family_stats()["families_uploaded"] == 1 and mgr.family_stats()["groups"] >= 1
    plain = vg.FontManager(True)
    plain.add_font_with_name("Two", [FIRA, NOTO])
    assert _render(vg, plain, r) == with_families and fid


def test_facade_damaged_glyf_tables_fall_back_to_the_host_reader(vg):
    """as test_damaged_glyf_tables_render_like_the_host_reader, through families: a group the device refuses is recorded by the
    host's reader and rendered again"""
    from pathlib import Path
    from conftest import FIRA
    from test_gpu_resident_fonts import _damage_glyf, _render
    rng = np.random.default_rng(7)
    font = Path(FIRA).read_bytes()
    r = vg.Renderer.new_precise(0)
    n_checked = n_fallbacks = n_ranges = 0
    for i in range(12):
        mutant = _damage_glyf(font, rng, n_hits=(1, 3, 40, 400)[i % 4])
        files = {}
        try:
            for way in ("families", "host"):
                mgr = _families_on(vg, "fonts") if way == "families" else vg.FontManager(True)
                if way == "host":
                    mgr.set_glyf_on_device(False)
                mgr.add_font_data(f"Mutant {i}", mutant)
                files[way] = _render(vg, mgr, r)
                if way == "families":
                    took_fallback, ranges = mgr.timings()["glyf_fallbacks"], mgr.family_stats()["groups"]
        except RuntimeError as e:
            assert way == "families" or "glyf" not in str(e), str(e)
            continue
        assert files["families"] == files["host"], i
        n_checked += 1
        n_fallbacks += took_fallback
        n_ranges += ranges
    assert n_checked >= 6 and n_fallbacks >= 1 and n_ranges >= n_checked
