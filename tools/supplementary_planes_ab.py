"""What the supplementary planes cost, every run on a fresh FontManager (the first render of a font id is what is measured), the
sides alternating in one process, best of --runs and median:
  the façade's first render_glyphs of the 20-file Noto Sans id and of Noto Sans Regular with vg_manager_set_supplementary_planes
    off and on (on: five, respectively two, more blocks and, with resident families, the plane-1 family stated by the host) —
    a copy of this file in a checkout of the parent commit, run with --parent, gives the parent's switch-off figures;
  vgsdf_family_tables_census over the font id's tables: the whole call and its kernel (HIP events);
  vgsdf_family_create_tables_at for plane 0 and plane 1 at the C ABI: the whole call, the count and the emit pass.
  python tools/supplementary_planes_ab.py [--runs 20] [--parent]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import NOTO, load_product, noto_files  # noqa: E402


def stats(v):
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms  worst {max(v) * 1e3:8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--parent", action="store_true", help="a checkout without the switch: the first renders alone")
    args = ap.parse_args()
    vg = load_product()
    inputs = [("Noto Sans, 20 files, one font id", noto_files()), ("Noto Sans Regular", [NOTO])]
    r = vg.Renderer.new_precise(0)

    def render_once(paths, on, families):
        mgr = vg.FontManager(True)
        if families:
            mgr.set_resident_fonts(True)
            mgr.set_resident_families(True)
        if on:
            mgr.set_supplementary_planes(True)
        mgr.add_font_with_name("Noto Sans Regular", paths)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        return time.perf_counter() - t0, len(w.files)

    sides = (False,) if args.parent else (False, True)
    for name, paths in inputs:
        for families in (False, True):
            for on in sides:
                render_once(paths, on, families)                                    # warm: code, allocator, clocks
            t, files = {s: [] for s in sides}, {}
            for _ in range(args.runs):
                for on in sides:
                    dt, files[on] = render_once(paths, on, families)
                    t[on].append(dt)
            print(f"\n{name}, {'resident families' if families else 'default forms'}, first render of a fresh manager, {args.runs} runs each, alternating")
            for on in sides:
                print(f"  switch {'on ' if on else 'off'} ({files[on]} files): {stats(t[on])}")
    if args.parent:
        return
    ctx = vg.SdfContext(0)
    for name, paths in inputs:
        mgr = vg.FontManager(True)
        fid = mgr.add_font_with_name("Noto Sans Regular", paths)
        descs = [mgr.family_tables_desc(fid, k) for k in range(len(paths))]
        fonts = [ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"]) for d in (mgr.resident_font_desc(fid, k) for k in range(len(paths)))]
        ctx.family_tables_census(descs)
        call, kernel = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            bits = ctx.family_tables_census(descs)
            call.append(time.perf_counter() - t0)
            kernel.append(ctx.family_census_kernel_ms() * 1e-3)
        n_blocks = sum(bin(int(w)).count("1") for w in bits)
        print(f"\n{name}: census over {len(paths)} faces, {n_blocks} blocks set")
        print(f"  the call {stats(call)}\n  its kernel {stats(kernel)}")
        for plane in (0, 1):
            ctx.family_create_tables_at(fonts, descs, plane).free()
        rows = {0: [], 1: []}
        for _ in range(args.runs):
            for plane in (0, 1):
                t0 = time.perf_counter()
                fam = ctx.family_create_tables_at(fonts, descs, plane)
                dt = time.perf_counter() - t0
                ms = ctx.family_tables_kernel_ms()
                rows[plane].append((dt, ms[0] * 1e-3, ms[1] * 1e-3, fam.count(0, 0xFFFF)))
                fam.free()
        for plane in (0, 1):
            v = rows[plane]
            print(f"  plane {plane}: {v[0][3]} entries | the call {stats([x[0] for x in v])}\n"
                  f"           count pass {stats([x[1] for x in v])}\n           emit pass  {stats([x[2] for x in v])}")
        for f in fonts:
            f.free()
    ctx.close()


if __name__ == "__main__":
    main()
