"""Resident fonts on the device: outlines uploaded once (vgsdf_font_create), glyphs rendered by (font, glyph id)
(vgsdf_outlines_submit_resident).

The output contract is equality with the glyf form (vgsdf_outlines_submit_glyf, itself pinned to the host's reader by
tests/test_gpu_glyf_decode.py) and with the goldens: rects, sizes, every segment bit for bit, every bitmap, the arena of the
in-place PBF form.  No tolerance appears anywhere.
"""
import hashlib

import numpy as np
import pytest

from conftest import FIRA, NOTO, noto_files
from test_golden_cpu import golden_rows

pytestmark = pytest.mark.gpu

E_ARG, E_GLYF = -1, -4   # vgsdf_status

SETS = {"fira": [FIRA], "noto_regular": [NOTO], "noto_all": None}


def _font_set(vg, which):
    paths = SETS[which] or noto_files()
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name("Font", paths)
    g = mgr.record_glyf_parts(fid)
    r = mgr.record_resident(fid)
    descs = [mgr.resident_font_desc(fid, k) for k in range(r["n_files"])]
    return mgr, fid, g, r, descs


def _upload(ctx, descs):
    return [ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"]) for d in descs]


def _glyf_subset(g, sel):
    """the glyf form built for the glyph list `sel` (indices into the recorded font, repeats allowed)"""
    parts_all, cmd_off = g["parts"], g["cmd_off"].astype(np.int64)
    first_part = np.searchsorted(parts_all["cmd_at"], cmd_off[:-1], side="left")
    last_part = np.searchsorted(parts_all["cmd_at"], cmd_off[1:], side="left")
    parts, new_off, store, at = [], [0], [], 0
    for gi in sel:
        p = parts_all[first_part[gi]:last_part[gi]].copy()
        p["cmd_at"] = (p["cmd_at"].astype(np.int64) - cmd_off[gi] + new_off[-1]).astype(np.uint32)
        for k in range(len(p)):
            ln = (int(p["byte_len"][k]) + 3) // 4 * 4
            store.append(g["bytes"][int(p["byte_off"][k]):int(p["byte_off"][k]) + ln])
            p["byte_off"][k] = at
            at += ln
        parts.append(p)
        new_off.append(new_off[-1] + int(cmd_off[gi + 1] - cmd_off[gi]))
    parts = np.concatenate(parts) if parts else parts_all[:0]
    store = np.concatenate(store) if store else np.zeros(0, np.uint8)
    return np.array(new_off, np.uint32), parts, store, g["scale"][sel], g["shift_x"][sel]


def _run_glyf(ctx, form, capacity, **pbf):
    ctx.outlines_submit_glyf(*form, capacity=capacity, **pbf)
    res = ctx.outlines_wait()
    at = ctx.outlines_pbf_positions() if pbf else None
    return res, ctx.outlines_segments(), at


def _run_resident(ctx, fonts, r, sel, capacity, **pbf):
    ctx.outlines_submit_resident(fonts, r["font_of"][sel], r["glyph_id"][sel], r["scale"][sel], r["shift_x"][sel], capacity=capacity, **pbf)
    res = ctx.outlines_wait()
    at = ctx.outlines_pbf_positions() if pbf else None
    return res, ctx.outlines_segments(), at


def _assert_same(a, b):
    (rects_a, bm_a, ob_a, ns_a), (so_a, segs_a), at_a = a
    (rects_b, bm_b, ob_b, ns_b), (so_b, segs_b), at_b = b
    assert ob_a == ob_b and ns_a == ns_b
    assert np.array_equal(rects_a, rects_b)
    assert np.array_equal(so_a, so_b) and segs_a.tobytes() == segs_b.tobytes()     # every segment, bit for bit
    assert bm_a is not None and bm_b is not None and len(bm_a) == len(bm_b)
    if at_a is None and at_b is None:
        assert np.array_equal(bm_a, bm_b)
    else:   # in-place PBF arena: the device writes the bitmaps only (the bytes between them are the caller's)
        assert np.array_equal(at_a, at_b)
        for at, w, h, has in zip(at_a, rects_a["w"], rects_a["h"], rects_a["has_raster"]):
            if has:
                lo, hi = int(at), int(at) + int(w) * int(h)
                assert hi <= len(bm_a) and bm_a[lo:hi].tobytes() == bm_b[lo:hi].tobytes()


@pytest.mark.parametrize("which", list(SETS))
def test_all_glyphs_by_id_equal_the_glyf_form_and_the_goldens(vg, which):
    _, _, g, r, descs = _font_set(vg, which)
    n = len(r["ids"])
    everything = np.arange(n)
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        assert all(f.device_bytes >= 48 * len(d["leaves"]) + len(d["bytes"]) + 4 * len(d["leaf_off"]) for f, d in zip(fonts, descs))
        want = _run_glyf(ctx, (g["cmd_off"], g["parts"], g["bytes"], g["scale"], g["shift_x"]), 8 << 20)
        cap = int(want[0][2]) + 64
        want = _run_glyf(ctx, (g["cmd_off"], g["parts"], g["bytes"], g["scale"], g["shift_x"]), cap)
        got = _run_resident(ctx, fonts, r, everything, cap)
        uploaded = ctx.resident_upload_bytes()
        _assert_same(got, want)
        # the same again (fonts stay resident, nothing about the first submission lingers)
        _assert_same(_run_resident(ctx, fonts, r, everything, cap), want)
        for f in fonts:
            f.free()
    finally:
        ctx.close()
    assert n > 1000 and uploaded <= 40 * n + 64 * len(descs) + 64
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


def test_subsets_repeats_single_blocks_and_mixed_faces(vg):
    _, _, g, r, descs = _font_set(vg, "noto_all")
    n = len(r["ids"])
    rng = np.random.default_rng(11)
    shuffled = rng.permutation(n)[:1500]
    shuffled = np.concatenate([shuffled, shuffled[:200], shuffled[[3, 3, 3]]])     # repeats, any order
    rng.shuffle(shuffled)
    block = np.flatnonzero(r["ids"] // 256 == int(r["ids"][n // 2]) // 256)         # one block's glyphs
    per_face = np.concatenate([np.flatnonzero(r["font_of"] == k)[:40] for k in range(r["n_files"])])   # all 20 faces in one submission
    mixed = rng.permutation(per_face)
    assert len(np.unique(r["font_of"][mixed])) == 20 and 0 < len(block) <= 256
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        for sel in (shuffled, block, mixed, np.array([int(block[0])])):
            want = _run_glyf(ctx, _glyf_subset(g, sel), 4 << 20)
            _assert_same(_run_resident(ctx, fonts, r, sel, 4 << 20), want)
        # a font list in another order than the faces' (font_of follows)
        order = np.arange(r["n_files"])[::-1]
        back = np.empty_like(order)
        back[order] = np.arange(len(order))
        r2 = dict(r, font_of=back[r["font_of"]].astype(np.uint16))
        _assert_same(_run_resident(ctx, [fonts[k] for k in order], r2, mixed, 4 << 20), _run_glyf(ctx, _glyf_subset(g, mixed), 4 << 20))
    finally:
        ctx.close()


def _varint_len(v):
    return np.where(v < 128, 1, np.where(v < 16384, 2, np.where(v < (1 << 21), 3, np.where(v < (1 << 28), 4, 5))))


def test_in_place_pbf_form(vg):
    _, _, g, r, descs = _font_set(vg, "noto_regular")
    n = len(r["ids"])
    pre = np.zeros(n, np.uint32)
    pre[np.flatnonzero(np.diff(np.concatenate([[-1], r["ids"] // 256])))] = 23     # room for a block header where a block opens
    fix = ((1 + _varint_len(r["ids"])) | ((1 + _varint_len(r["advances"])) << 4)).astype(np.uint8)
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        form = (g["cmd_off"], g["parts"], g["bytes"], g["scale"], g["shift_x"])
        probe = _run_glyf(ctx, form, 8 << 20, pbf_pre=pre, pbf_fix=fix)
        cap = int(probe[0][2]) + 64

        want = _run_glyf(ctx, form, cap, pbf_pre=pre, pbf_fix=fix)
        got = _run_resident(ctx, fonts, r, np.arange(n), cap, pbf_pre=pre, pbf_fix=fix)
        _assert_same(got, want)
        # (the arena holds the entries' headers and the reserved bytes besides the bitmaps)
        assert int(got[0][2]) > int(_run_resident(ctx, fonts, r, np.arange(n), cap)[0][2]) + 23
    finally:
        ctx.close()


def test_upload_size_depends_on_the_counts_alone(vg):
    """two submissions of equally many glyphs with different outlines upload the same number of bytes, at most
    40 n_glyphs + 64 n_fonts + 64 (the layout is 33 n + 8 with the PBF arrays, 28 n + 8 without, + 32 per font; the glyf form's
    smallest figure is 184 bytes per glyph)"""
    _, _, g, r, descs = _font_set(vg, "noto_regular")
    slots = np.diff(g["cmd_off"].astype(np.int64))
    order = np.argsort(slots)
    light, heavy = order[:500], order[-500:]
    assert slots[heavy].sum() > 4 * slots[light].sum() + 1000
    ctx = vg.SdfContext(0)
    try:
        fonts = _upload(ctx, descs)
        sizes = []
        for sel in (light, heavy):
            _run_resident(ctx, fonts, r, sel, 4 << 20)
            sizes.append(ctx.resident_upload_bytes())
        assert sizes[0] == sizes[1] and 0 < sizes[0] <= 40 * 500 + 64 * 1 + 64
        glyf_block = 20 * 500 + 48 * int((np.diff(np.searchsorted(g["parts"]["cmd_at"], g["cmd_off"]))[heavy]).sum())
        assert sizes[1] < glyf_block
    finally:
        ctx.close()


def test_a_font_is_shared_by_the_contexts_of_its_device(vg):
    _, _, g, r, descs = _font_set(vg, "fira")
    n = len(r["ids"])
    a, b = vg.SdfContext(0), vg.SdfContext(0)
    try:
        fonts = _upload(a, descs)                       # created through one context ...
        want = _run_glyf(a, (g["cmd_off"], g["parts"], g["bytes"], g["scale"], g["shift_x"]), 4 << 20)
        half = np.arange(n // 2)
        rest = np.arange(n // 2, n)
        # ... named by two, both in flight at once
        a.outlines_submit_resident(fonts, r["font_of"][half], r["glyph_id"][half], r["scale"][half], r["shift_x"][half], capacity=4 << 20)
        b.outlines_submit_resident(fonts, r["font_of"][rest], r["glyph_id"][rest], r["scale"][rest], r["shift_x"][rest], capacity=4 << 20)
        ra, rb = a.outlines_wait(), b.outlines_wait()
        assert np.array_equal(np.concatenate([ra[0], rb[0]]), want[0][0])
        assert np.array_equal(np.concatenate([ra[1], rb[1]]), want[0][1])
        for f in fonts:
            f.free()
    finally:
        a.close()
        b.close()


def test_bad_descriptions_and_bad_submissions_are_refused(vg):
    _, _, g, r, descs = _font_set(vg, "fira")
    d = descs[0]
    n = len(r["ids"])
    composite = int(np.flatnonzero(np.diff(d["leaf_off"].astype(np.int64)) > 1)[0])
    ctx = vg.SdfContext(0)
    try:
        def refused(leaf_off=None, leaves=None, store=None):
            with pytest.raises(vg.VgsdfError) as e:
                ctx.font_create(d["leaf_off"] if leaf_off is None else leaf_off, d["leaves"] if leaves is None else leaves,
                                d["bytes"] if store is None else store)
            assert e.value.code == E_ARG

        bad = d["leaf_off"].copy()
        bad[5], bad[6] = bad[6] + 1, bad[5]                       # not ascending
        refused(leaf_off=bad)
        bad = d["leaf_off"].copy()
        bad[-1] += 1                                               # does not end at n_leaves
        refused(leaf_off=bad)
        bad = d["leaves"].copy()
        k = int(np.argmax(bad["byte_off"].astype(np.int64) + bad["byte_len"]))
        bad["byte_len"][k] += 8                                    # a leaf past `bytes`
        refused(leaves=bad)
        bad = d["leaves"].copy()
        bad["byte_off"][k] += 2                                    # not 4-aligned
        refused(leaves=bad)
        bad = d["leaves"].copy()
        bad["cmd_at"][int(d["leaf_off"][composite]) + 1] += 1      # leaves that do not tile their glyph's slots
        refused(leaves=bad)
        bad = d["leaves"].copy()
        bad["n_contours"][0] = 0
        refused(leaves=bad)
        refused(store=d["bytes"][:-2])                             # n_bytes not a multiple of 4

        fonts = _upload(ctx, descs)
        everything = np.arange(n)

        def bad_submission(**change):
            args = dict(font_of=r["font_of"], glyph_id=r["glyph_id"])
            args.update(change)
            with pytest.raises(vg.VgsdfError) as e:
                ctx.outlines_submit_resident(fonts, args["font_of"], args["glyph_id"], r["scale"], r["shift_x"], capacity=4 << 20)
            assert e.value.code == E_ARG

        ids = r["glyph_id"].copy()
        ids[7] = len(d["leaf_off"]) - 1                            # a glyph id past the face
        bad_submission(glyph_id=ids)
        fo = r["font_of"].copy()
        fo[n - 1] = 1                                              # font_of past n_fonts
        bad_submission(font_of=fo)
        # the context renders a good submission afterwards
        want = _run_glyf(ctx, (g["cmd_off"], g["parts"], g["bytes"], g["scale"], g["shift_x"]), 4 << 20)
        _assert_same(_run_resident(ctx, fonts, r, everything, 4 << 20), want)
        # a glyph id without leaves is a glyph without outline
        empty = int(np.flatnonzero(np.diff(d["leaf_off"].astype(np.int64)) == 0)[0])
        ctx.outlines_submit_resident(fonts, [0, 0], [empty, int(r["glyph_id"][40])], r["scale"][:2], r["shift_x"][:2], capacity=1 << 20)
        rects, _, _, _ = ctx.outlines_wait()
        assert rects["has_raster"][0] == 0 and rects["n_segments"][0] == 0
    finally:
        ctx.close()


def test_an_entry_the_decoder_refuses_fails_the_batch_as_in_the_glyf_form(vg):
    """a leaf with fewer slots than its entry needs: VGSDF_E_GLYF from wait (the error word the glyf form raises), and the
    context goes on"""
    _, _, g, r, descs = _font_set(vg, "fira")
    d = descs[0]
    lv = d["leaves"].copy()
    single = np.flatnonzero(np.diff(d["leaf_off"].astype(np.int64)) == 1)
    single = single[np.isin(single, r["glyph_id"])]               # (glyph ids the font's code points reach)
    gid = int(single[np.argmax(lv["cmd_cap"][d["leaf_off"][single]])])
    k = int(d["leaf_off"][gid])
    assert lv["cmd_cap"][k] > 8
    lv["cmd_cap"][k] -= 5                                          # (alone in its glyph: the tiling still holds)
    ctx = vg.SdfContext(0)
    try:
        short = ctx.font_create(d["leaf_off"], lv, d["bytes"])
        good = ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"])
        ctx.outlines_submit_resident([short], r["font_of"], r["glyph_id"], r["scale"], r["shift_x"], capacity=4 << 20)
        with pytest.raises(vg.VgsdfError) as e:
            ctx.outlines_wait()
        assert e.value.code == E_GLYF
        want = _run_glyf(ctx, (g["cmd_off"], g["parts"], g["bytes"], g["scale"], g["shift_x"]), 4 << 20)
        _assert_same(_run_resident(ctx, [good], r, np.arange(len(r["ids"])), 4 << 20), want)
    finally:
        ctx.close()


# ---- the host façade with the switch on ----

def _pbf_shas(files):
    return {k.split("/", 1)[1].split("-")[0]: hashlib.sha256(v).hexdigest() for k, v in files.items()}


def _render(vg, mgr, r):
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place_pbf", "packed_bitmaps"])
@pytest.mark.parametrize("key", ["fira", "noto_regular", "noto_all"])
def test_facade_writes_the_golden_files_from_resident_fonts(vg, key, in_place):
    import json
    from conftest import GOLDEN
    from test_golden_cpu import set_paths
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())[key]
    name, paths = set_paths(key)
    r = vg.Renderer.new_precise(0)
    mgr = vg.FontManager(True)
    mgr.set_resident_fonts(True)
    mgr.set_in_place_pbf(in_place)
    mgr.add_font_with_name(name, paths)
    first = _render(vg, mgr, r)
    t1, s1 = mgr.timings(), mgr.resident_stats()
    second = _render(vg, mgr, r)
    t2, s2 = mgr.timings(), mgr.resident_stats()
    assert _pbf_shas(first) == golden and second == first
    # every group resident, the faces uploaded on the first render and nothing of a font on the second
    assert s1["groups"] == t1["fe_groups"] >= 1 and t1["glyf_groups"] == 0 and t1["glyf_fallbacks"] == 0
    assert s1["fonts_uploaded"] == len(paths) and s1["font_bytes"] > 0
    assert s2["groups"] == t2["fe_groups"] == s1["groups"] and s2["fonts_uploaded"] == 0 and s2["font_bytes"] == 0 and t2["glyf_fallbacks"] == 0
    assert 0 < s2["block_bytes"] <= 40 * t2["glyphs"] + 64 * len(paths) * s2["groups"] + 64 * s2["groups"]
    # a manager of its own on the same renderer finds the copies of ITS faces missing (they are keyed per face) and uploads them
    # once; preloading makes the first render warm
    other = vg.FontManager(True)
    other.set_resident_fonts(True)
    other.add_font_with_name(name, paths)
    assert r.preload_fonts(other) > 0 and r.preload_fonts(other) == 0
    assert _render(vg, other, r) == first and other.resident_stats()["fonts_uploaded"] == 0


def test_facade_lanes_that_share_a_device_and_single_blocks(vg):
    import json
    from conftest import GOLDEN
    from test_golden_cpu import set_paths
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())
    name, paths = set_paths("noto_all")
    r = vg.Renderer.new_multi([0, 0])
    mgr = vg.FontManager(True)
    mgr.set_resident_fonts(True)
    mgr.set_lane_form(2)   # hybrid: whole (font, block) tasks, the heaviest blocks split between the lanes
    fid = mgr.add_font_with_name(name, paths)
    files = _render(vg, mgr, r)
    s, t = mgr.resident_stats(), mgr.timings()
    assert _pbf_shas(files) == golden["noto_all"]
    assert s["groups"] == t["fe_groups"] >= 2 and t["glyf_groups"] == 0 and t["glyf_fallbacks"] == 0
    assert s["fonts_uploaded"] == len(paths)          # one copy per (device, face): the two lanes share them
    files2 = _render(vg, mgr, r)
    assert files2 == files and mgr.resident_stats()["font_bytes"] == 0
    # single blocks on demand (vg_manager_render_blocks): the fonts are on the device already
    single = vg.Renderer.new_precise(0)
    one = vg.FontManager(True)
    one.set_resident_fonts(True)
    fid = one.add_font_with_name(name, paths)
    for k, starts in enumerate(([0], [1024], [0x0900, 0x1000, 0])):
        w = vg.DummyWriter()
        one.render_glyphs(w, single, fid, starts)
        got = _pbf_shas(w.files)
        assert got == {str(b): golden["noto_all"][str(b)] for b in starts}
        st = one.resident_stats()
        assert st["groups"] >= 1 and (st["fonts_uploaded"] == len(paths)) == (k == 0) and one.timings()["glyf_fallbacks"] == 0


def test_budget_zero_keeps_the_glyf_form(vg):
    from test_golden_cpu import set_paths
    name, paths = set_paths("fira")
    files = {}
    for budget in (None, 0):
        r = vg.Renderer.new_precise(0)
        if budget is not None:
            r.set_resident_budget(budget)
        mgr = vg.FontManager(True)
        mgr.set_resident_fonts(True)
        mgr.add_font_with_name(name, paths)
        files[budget] = _render(vg, mgr, r)
        s, t = mgr.resident_stats(), mgr.timings()
        if budget == 0:
            assert s == {"groups": 0, "fonts_uploaded": 0, "font_bytes": 0, "block_bytes": 0} and t["glyf_groups"] == t["fe_groups"] >= 1
        else:
            assert s["groups"] == t["fe_groups"] >= 1
    assert files[0] == files[None]


def _damage_glyf(font: bytes, rng, n_hits: int) -> bytes:
    """random bytes inside the glyf table (flags, coordinates, end points, component records)"""
    n_tables = int.from_bytes(font[4:6], "big")
    for i in range(n_tables):
        rec = 12 + 16 * i
        if font[rec:rec + 4] == b"glyf":
            off, ln = int.from_bytes(font[rec + 8:rec + 12], "big"), int.from_bytes(font[rec + 12:rec + 16], "big")
            b = bytearray(font)
            for pos in rng.integers(0, ln, n_hits):
                b[off + int(pos)] = int(rng.integers(0, 256))
            return bytes(b)
    raise AssertionError("no glyf table")


def test_damaged_glyf_tables_render_like_the_host_reader(vg):
    """the error-word paths the device has for the glyf form, reached from resident fonts: where an entry's arrays do not fit,
    the batch is flagged and recorded with the host's reader; everywhere else both read the same damaged bytes the same way"""
    from pathlib import Path
    rng = np.random.default_rng(7)
    font = Path(FIRA).read_bytes()
    r = vg.Renderer.new_precise(0)
    n_checked = n_fallbacks = n_resident = 0
    for i in range(12):
        mutant = _damage_glyf(font, rng, n_hits=(1, 3, 40, 400)[i % 4])
        files = {}
        took_fallback = resident = 0
        try:
            for way in ("resident", "host"):
                mgr = vg.FontManager(True)
                if way == "resident":
                    mgr.set_resident_fonts(True)
                else:
                    mgr.set_glyf_on_device(False)
                mgr.add_font_data(f"Mutant {i}", mutant)
                files[way] = _render(vg, mgr, r)
                if way == "resident":
                    took_fallback = mgr.timings()["glyf_fallbacks"]
                    resident = mgr.resident_stats()["groups"]
        except RuntimeError as e:
            # absurd coordinates can make the front-end refuse a batch ("a glyph flattens to more than 2^28 points ..."):
            # then both ways refuse it
            assert way == "resident" or "glyf" not in str(e), str(e)
            continue
        assert files["resident"] == files["host"], i
        n_checked += 1
        n_fallbacks += took_fallback
        n_resident += resident
    assert n_checked >= 6 and n_resident >= 1 and 1 <= n_fallbacks < n_checked   # at least one mutant took the fallback, at least one did not
