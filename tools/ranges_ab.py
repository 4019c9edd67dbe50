#!/usr/bin/env python3
"""A/B of the two submissions that name glyphs of resident fonts, at the C ABI: vgsdf_outlines_submit_resident (33 bytes per
glyph, gathered by the host) against vgsdf_outlines_submit_ranges (code-point ranges of a resident family, one task per
256-code-point block; with pbf_pre the device also writes the PBF entry bytes).  Same context, same fonts, the two forms
interleaved; per form the host time of the submit call (what the calling thread spends building and enqueueing), the time from
submit to the end of wait, and the block uploaded.  Prints one table; needs a GPU.

    python tools/ranges_ab.py [--reps 200] [--out profiles/resident_families_ab.txt]
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from conftest import FIRA, NOTO, load_product, noto_files  # noqa: E402


def varint_len(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def measure(vg, name, paths, commands, reps, lines):
    from versatiles_glyphs_rs_amd.device import RECT_DTYPE, _COutlinesRanges, _COutlinesResident
    L = vg.load_library()
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name("Font", paths)
    r = mgr.record_resident_commands(fid) if commands else mgr.record_resident(fid)
    ctx = vg.SdfContext(0)
    if commands:
        fonts = [ctx.font_create_commands(*[mgr.command_font_desc(fid, k)[a] for a in ("cmd_off", "dat_off", "kinds", "coords")]) for k in range(r["n_files"])]
    else:
        fonts = [ctx.font_create(*[mgr.resident_font_desc(fid, k)[a] for a in ("leaf_off", "leaves", "bytes")]) for k in range(r["n_files"])]
    fam = ctx.family_create(fonts, r["ids"], r["font_of"], r["glyph_id"], r["advances"], r["scale"], r["shift_x"])
    n = len(r["ids"])
    blocks = np.array(sorted(set((r["ids"] // 256).tolist())))
    first, last = (blocks * 256).astype(np.uint16), (blocks * 256 + 255).astype(np.uint16)
    task_pre = np.full(len(blocks), 24, np.uint32)
    glyph_pre = np.zeros(n, np.uint32)
    glyph_pre[np.searchsorted(r["ids"], blocks * 256)] = 24
    fix = np.array([(1 + varint_len(int(i))) | ((1 + varint_len(int(a))) << 4) for i, a in zip(r["ids"], r["advances"])], np.uint8)
    handles = (C.c_void_p * len(fonts))(*[f._h for f in fonts])
    fams = (C.c_void_p * 1)(fam._h)
    fam_of = np.zeros(len(blocks), np.uint16)
    cap = 96 << 20
    out = L.vgsdf_host_alloc(cap)
    rects = np.zeros(n, dtype=RECT_DTYPE)
    ob, ns, done = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    for pbf in (False, True):
        res = _COutlinesResident(n, len(fonts), C.cast(handles, C.c_void_p), r["font_of"].ctypes.data, r["glyph_id"].ctypes.data,
                                 r["scale"].ctypes.data, r["shift_x"].ctypes.data, glyph_pre.ctypes.data if pbf else None,
                                 fix.ctypes.data if pbf else None)
        rng = _COutlinesRanges(len(blocks), 1, C.cast(fams, C.c_void_p), fam_of.ctypes.data, first.ctypes.data, last.ctypes.data,
                               task_pre.ctypes.data if pbf else None)
        forms = (("resident", L.vgsdf_outlines_submit_resident, res), ("ranges", L.vgsdf_outlines_submit_ranges, rng))
        t_submit = {k: [] for k, _, _ in forms}
        t_total = {k: [] for k, _, _ in forms}
        upload = {}
        for rep in range(reps + 20):                      # (the first 20 rounds warm the context's buffers and guesses)
            for key, fn, co in forms:
                t0 = time.perf_counter()
                rc = fn(ctx._h, C.byref(co), out, cap)
                t1 = time.perf_counter()
                rc2 = L.vgsdf_outlines_wait(ctx._h, rects.ctypes.data, C.byref(ob), C.byref(ns), C.byref(done))
                t2 = time.perf_counter()
                assert rc == 0 and rc2 == 0 and done.value == 1, (key, rc, rc2, L.vgsdf_last_error(ctx._h))
                upload[key] = int(L.vgsdf_outlines_resident_upload_bytes(ctx._h))
                if rep >= 20:
                    t_submit[key].append(t1 - t0)
                    t_total[key].append(t2 - t0)
        for key, _, _ in forms:
            s, t = np.array(t_submit[key]) * 1e6, np.array(t_total[key]) * 1e6
            lines.append(f"{name:14s} {'commands' if commands else 'glyf':8s} {'pbf' if pbf else 'packed':6s} {key:8s} glyphs {n:6d} tasks {len(blocks):4d} "
                         f"upload {upload[key]:8d} B  submit call median {np.median(s):7.1f} us (p10 {np.percentile(s, 10):7.1f})  "
                         f"submit..wait median {np.median(t):7.1f} us (p10 {np.percentile(t, 10):7.1f})  arena {ob.value} B")
            print(lines[-1], flush=True)
    L.vgsdf_host_free(out)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vg = load_product()
    if vg.device_count() < 1:
        raise SystemExit("no HIP device: this measurement has no CPU form")
    lines = []
    for name, paths in (("fira", [FIRA]), ("noto_regular", [NOTO]), ("noto_20_files", noto_files())):
        for commands in (False, True):
            measure(vg, name, paths, commands, a.reps, lines)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
