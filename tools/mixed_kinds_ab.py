#!/usr/bin/env python3
"""A/B of the façade's mixed stores (vg_manager_set_mixed_stores) on groups that hold glyphs of `glyf` files and of CFF files:
switch off — today's form, command stores of ALL files, the `glyf` files' built by the host's reader — against switch on — a glyf
store per `glyf` file, a command store per other file, one submission against both kinds.  Switches otherwise: the device's glyf
decoder, resident fonts, resident commands 1; by glyph names and as ranges of families.

Inputs: `both` (Fira's first 400 glyph ids as CFF in front of Fira Sans, one font id), `noto_cff` (the same CFF file in front of
the 20 Noto Sans files, one font id), `two_ids` (Fira Sans and the CFF file under font ids of their own, one group).

Per input, mode and repetition a fresh renderer and a fresh manager: wall time and vg_timings of the FIRST render (stores and
families are built) and of a SECOND render (everything resident); the two modes alternate.  Medians over the repetitions.  A
checkout without the switch (the parent commit) measures the "off" column alone.  Needs a GPU.

    python tools/mixed_kinds_ab.py [--reps 15] [--only both] [--out profiles/mixed_kinds_ab.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from conftest import FIRA, load_product, noto_files  # noqa: E402

PHASES = ("tessellate_s", "pack_s", "device_s", "encode_s", "total_s")


def manager(vg, fonts, families, mixed):
    mgr = vg.FontManager(True)
    mgr.set_glyf_on_device(True)
    mgr.set_resident_fonts(True)
    mgr.set_resident_commands(1)
    mgr.set_resident_families(bool(families))
    if mixed:
        mgr.set_mixed_stores(True)
    for name, paths in fonts:
        mgr.add_font_with_name(name, paths)
    return mgr


def one(vg, fonts, families, mixed):
    """-> [(wall seconds, timings)] of the first and the second render, and the files' total bytes"""
    r = vg.Renderer.new_precise(0)
    mgr = manager(vg, fonts, families, mixed)
    out = []
    for _ in range(2):
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        wall = time.perf_counter() - t0
        form = ("mixed %d " % mgr.mixed_stats()["groups"] if mixed is not None and hasattr(mgr, "mixed_stats") else "") + "family %d command %d glyf-named %d" % (
            mgr.family_stats()["groups"], mgr.command_stats()["groups"], mgr.resident_stats()["groups"])
        out.append((wall, mgr.timings(), form))
    size = sum(len(v) for v in w.files.values())
    r.close()
    return out, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vg = load_product()
    if vg.device_count() < 1:
        raise SystemExit("no HIP device: this measurement has no CPU form")
    from fira_cff_kit import fira_as_cff
    import tempfile
    tmp = Path(tempfile.mkdtemp()) / "Fira Sans CFF 400 - Regular.otf"
    tmp.write_bytes(fira_as_cff(400))
    inputs = {"both": [("Fira Sans Regular", [tmp, FIRA])], "noto_cff": [("Noto Sans Regular", [tmp] + noto_files())],
              "two_ids": [("Fira Sans Regular", [FIRA]), ("Fira Sans CFF Regular", [tmp])]}
    has_switch = hasattr(vg.FontManager, "set_mixed_stores")
    modes = (False, True) if has_switch else (False,)
    lines = [f"mixed stores A/B: {a.reps} repetitions, fresh renderer and manager each, modes alternating; medians, microseconds"
             + ("" if has_switch else "  (this checkout has no switch: off only)")]
    for name, fonts in inputs.items():
        if a.only and name != a.only:
            continue
        for families in (0, 1):
            got = {m: [] for m in modes}
            one(vg, fonts, families, False)                  # (warms the process: code objects, the pool)
            for _ in range(a.reps):
                for m in modes:
                    got[m].append(one(vg, fonts, families, m))
            for m in modes:
                for which, label in ((0, "first render (stores built)"), (1, "second render (resident)")):
                    wall = np.median([g[0][which][0] for g in got[m]]) * 1e6
                    ph = {k: np.median([g[0][which][1][k] for g in got[m]]) * 1e6 for k in PHASES}
                    t, form = got[m][-1][0][which][1], got[m][-1][0][which][2]
                    lines.append(f"{name:9s} {'ranges' if families else 'named ':6s} switch {'on ' if m else 'off'} {label:28s} wall {wall:9.1f}  "
                                 + "  ".join(f"{k[:-2]} {ph[k]:8.1f}" for k in PHASES)
                                 + f"  glyphs {t['glyphs']} groups {t['fe_groups']} ({form}) bytes {got[m][-1][1]}")
                    print(lines[-1], flush=True)
            if has_switch:
                assert got[False][-1][1] == got[True][-1][1]
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
