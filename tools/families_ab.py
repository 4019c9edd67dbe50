#!/usr/bin/env python3
"""A/B of the façade with resident families off and on (vg_manager_set_resident_families), end to end: fonts -> PBF bytes into a
NULL sink on one renderer, the modes alternating render by render in one process.  Per workload and mode: best and median
wall time of a render, the calling thread's tessellate_s + pack_s + encode_s (vg_timings) of the median render, the bytes of
the submissions' upload blocks, the sustained rate over a window of back-to-back renders and, from a run of its own with
VGSDF_TRACE set (a fresh child process, the modes one after the other), the device span of the submissions.  Needs a GPU.

    python tools/families_ab.py [--reps 40] [--sustain 1.0] [--span 30] [--tag branch] [--product DIR] [--out FILE]

--product DIR: the package directory (versatiles-glyphs-rs_amd/, built) of ANOTHER checkout, so that the parent commit is
measured by this same script; a library without vg_manager_set_resident_families gives the "off" rows only.  Alternate the two
commands, parent and branch, a few times in one session and keep every row: --out appends.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from conftest import FIRA, NOTO, load_product, noto_files  # noqa: E402

WORKLOADS = ("noto_regular", "noto_20_files", "21_fonts")


def product(path):
    if not path:
        return load_product()
    pkg = Path(path).resolve()
    name = "versatiles_glyphs_rs_amd"
    spec = importlib.util.spec_from_file_location(name, pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def modes(vg):
    has = hasattr(vg.FontManager, "set_resident_families")
    return tuple((s, f) for s in ("fonts", "commands") for f in ((False, True) if has else (False,)))


def manager(vg, workload, store, families):
    m = vg.FontManager(True)
    if store == "fonts":
        m.set_resident_fonts(True)
    else:
        m.set_resident_commands(2)
    if families:
        m.set_resident_families(True)
    if workload == "noto_regular":
        m.add_font_with_name("Noto Sans Regular", [NOTO])
    elif workload == "noto_20_files":
        m.add_font_with_name("Noto Sans", noto_files())
    else:
        for i, p in enumerate([FIRA] + list(noto_files())):
            m.add_font_with_name(f"Font {i:02d}", [p])
    return m


def span_child(a):
    """under VGSDF_TRACE: every (workload, mode) by itself, a marker on stderr in front of its submissions' span lines"""
    vg = product(a.product)
    r = vg.Renderer.new_precise(0)
    for workload in WORKLOADS:
        for store, fam in modes(vg):
            m = manager(vg, workload, store, fam)
            for phase, n in (("warm", 5), ("timed", a.span)):
                sys.stderr.write(f"[ab] {workload} {store} {int(fam)} {phase}\n")
                sys.stderr.flush()
                for _ in range(n):
                    m.render_glyphs(None, r)


def spans(a):
    """{(workload, store, fam): (median, min) of the device spans in us, submissions per render}"""
    cp = subprocess.run([sys.executable, __file__, "--span-child", "--span", str(a.span)] + (["--product", a.product] if a.product else []),
                        env=dict(os.environ, VGSDF_TRACE="1"), capture_output=True, text=True)
    if cp.returncode != 0:
        raise SystemExit(f"span run failed ({cp.returncode}): {cp.stderr[-2000:]}")
    out, key = {}, None
    for line in cp.stderr.splitlines():
        if line.startswith("[ab] "):
            w, s, f, phase = line.split()[1:]
            key = (w, s, f == "1") if phase == "timed" else None
        elif key and (m := re.search(r"device span of the submission.*?: ([0-9.]+) us", line)):
            out.setdefault(key, []).append(float(m.group(1)))
    return {k: (float(np.median(v)), min(v), len(v) / a.span) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--sustain", type=float, default=1.0)
    ap.add_argument("--span", type=int, default=30)
    ap.add_argument("--tag", default="branch")
    ap.add_argument("--product", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--span-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.span_child:
        return span_child(a)
    vg = product(a.product)
    if vg.device_count() < 1:
        raise SystemExit("no HIP device: this measurement has no CPU form")
    MODES = modes(vg)
    r = vg.Renderer.new_precise(0)
    rows = []
    for workload in WORKLOADS:
        mgrs = [manager(vg, workload, s, f) for s, f in MODES]
        for m in mgrs:                                   # uploads, buffers and guesses
            for _ in range(5):
                m.render_glyphs(None, r)
        wall = [[] for _ in MODES]
        host = [[] for _ in MODES]
        for _ in range(a.reps):
            for k, m in enumerate(mgrs):
                t = time.perf_counter()
                m.render_glyphs(None, r)
                wall[k].append(time.perf_counter() - t)
                tm = m.timings()
                host[k].append(tm["tessellate_s"] + tm["pack_s"] + tm["encode_s"])
        for k, (m, (store, fam)) in enumerate(zip(mgrs, MODES)):
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < a.sustain:
                m.render_glyphs(None, r)
                n += 1
            rate = n * m.timings()["glyphs"] / (time.perf_counter() - t0)
            st = m.family_stats() if fam else (m.resident_stats() if store == "fonts" else m.command_stats())
            w, h = np.array(wall[k]) * 1e6, np.array(host[k]) * 1e6
            rows.append(((workload, store, fam),
                         f"{a.tag:7s} {workload:14s} {store:8s} families {'on ' if fam else 'off'} glyphs {m.timings()['glyphs']:6d} groups {st['groups']:2d} "
                         f"block {st['block_bytes']:8d} B  render best {w.min():7.1f} us median {np.median(w):7.1f} us  "
                         f"tessellate+pack+encode median {np.median(h):6.1f} us (best {h.min():6.1f})  sustained {rate / 1e6:6.2f} M glyphs/s"))
    del r
    sp = spans(a) if a.span > 0 else {}
    lines = []
    for key, text in rows:
        if key in sp:
            text += f"  device span median {sp[key][0]:6.1f} us (min {sp[key][1]:6.1f}; {sp[key][2]:.0f} per render)"
        lines.append(text)
        print(text, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
