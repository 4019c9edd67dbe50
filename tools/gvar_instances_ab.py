"""Timings of variable glyf + gvar instances, medians of --runs, every run on a fresh FontManager (so the face's command table
is built in the timed span):
  (1) the build of an instance's command store, alternating between
        host    Face::command_table() (through vg_manager_command_font_desc: the gvar walk, deltas and inferred points for every
                glyph id) plus vgsdf_font_create_commands of it, and
        device  vgsdf_font_create_gvar of the face's loca, glyf and gvar (the whole call, and its count / deltas / emit passes by
                HIP events),
      and, for scale, the command table of the same file added plainly (the static walk).  Needs a device;
  (2) --static [--root CHECKOUT --label NAME]: the command table and the recorded outlines of static files (Fira Sans, Noto Sans
      Regular) with the package of CHECKOUT (default: this one), for an A/B between two checkouts — run the two in turn, process
      by process.  No device.
Inputs of (1): the 315-glyph fixtures of tests/gvar_instances_kit.py (sheared second master, pure-scale second master, two axes).
  python tools/gvar_instances_ab.py [--runs 21] [--static [--root ../parent --label parent]]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def stats(v):
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--root", default=str(HERE), help="with --static: the checkout whose package is measured")
    ap.add_argument("--label", default="head", help="with --static: what the lines call that checkout")
    args = ap.parse_args()
    root = Path(args.root).resolve() if args.static else HERE
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "tests"))
    from conftest import FIRA, NOTO, load_product
    vg = load_product()

    def table_once(data, loc):
        mgr = vg.FontManager(False)
        fid = mgr.add_font_data("Timed", data) if loc is None else mgr.add_font_instance("Timed", data, loc)
        t0 = time.perf_counter()
        n = len(mgr.command_font_desc(fid)["kinds"])
        return time.perf_counter() - t0, n

    if args.static:
        for name, path in (("Fira Sans", FIRA), ("Noto Sans Regular", NOTO)):
            data = Path(path).read_bytes()
            tables, records = [], []
            for _ in range(args.runs):
                tables.append(table_once(data, None)[0])
                mgr = vg.FontManager(False)
                fid = mgr.add_font_data("Timed", data)
                t0 = time.perf_counter()
                mgr.record_outlines(fid)
                records.append(time.perf_counter() - t0)
            print(f"{args.label:7s} {name:18s} command table {stats(tables)}   record_outlines {stats(records)}")
        return
    import gvar_instances_kit as G
    ctx = vg.SdfContext(0)
    for kind, loc in (("shear", {"wght": 650}), ("scale", {"wght": 650}), ("two_axes", G.EXACT_TWO_AXES[1])):
        data = G.variable_glyf_fira(kind)
        table, upload, device, passes, plain, n = [], [], [], [], [], 0
        for run in range(args.runs + 1):
            mgr = vg.FontManager(False)
            fid = mgr.add_font_instance("Timed", data, loc)
            t0 = time.perf_counter()
            host = mgr.command_font_desc(fid)
            t1 = time.perf_counter()
            f = ctx.font_create_commands(host["cmd_off"], host["dat_off"], host["kinds"], host["coords"])
            t2 = time.perf_counter()
            f.free()
            desc = vg.FontManager(False)
            desc = desc.gvar_font_desc(desc.add_font_instance("Timed", data, loc))
            t3 = time.perf_counter()
            f = ctx.font_create_gvar(desc)
            t4 = time.perf_counter()
            f.free()
            if run:          # (the first round pays for the context's scratch and the code objects' load)
                table.append(t1 - t0), upload.append(t2 - t1), device.append(t4 - t3), passes.append(ctx.font_gvar_kernel_ms())
                plain.append(table_once(data, None)[0])
            n = len(host["kinds"])
        ms = [statistics.median(p[i] for p in passes) for i in range(3)]
        print(f"{kind:9s} {n:6d} commands   host: table {stats(table)}  + create_commands {stats(upload)}")
        print(f"{'':9s} {'':6s}            device: create_gvar {stats(device)}  (passes, median: count {ms[0]:.3f}  deltas {ms[1]:.3f}  emit {ms[2]:.3f} ms)")
        print(f"{'':9s} {'':6s}            added plainly: table {stats(plain)}")
    ctx.close()


if __name__ == "__main__":
    main()
