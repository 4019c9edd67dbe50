"""Timings of the command stores of N instances of ONE variable glyf + gvar file, medians of --runs, three sides alternating in
one process, every round on fresh FontManagers (so the host's command tables are built in the timed span):
  host     N x ( Face::command_table() through vg_manager_command_font_desc  +  vgsdf_font_create_commands of it )
  single   N x vgsdf_font_create_gvar of the face's loca, glyf and gvar at the instance's position
  batched  one vgsdf_fonts_create_gvar over the N positions (the whole call, and its count / deltas / emit passes by HIP events)
Inputs: the 315-glyph fixtures of tests/gvar_instances_kit.py (sheared second master, pure-scale second master, two axes) at
N = 1, 3, 9 positions spread over the weight axis (two axes: weight and width together).  Per side the time of the N stores and
the time per instance.  Needs a device.
  python tools/gvar_batch_ab.py [--runs 21]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def locations(kind, n):
    """n positions off the default, evenly spread"""
    out = []
    for k in range(n):
        t = (k + 1) / n
        loc = {"wght": 400 + 500 * t}
        if kind == "two_axes":
            loc["wdth"] = 100 + 100 * t
        out.append(loc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    args = ap.parse_args()
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE / "tests"))
    from conftest import load_product
    vg = load_product()
    import gvar_instances_kit as G
    ctx = vg.SdfContext(0)
    med = lambda v: statistics.median(v) * 1e3  # noqa: E731
    for kind in ("shear", "scale", "two_axes"):
        data = G.variable_glyf_fira(kind)
        for n in (1, 3, 9):
            locs = locations(kind, n)
            host, single, batched, passes = [], [], [], []
            for run in range(args.runs + 1):
                # host: the table of every instance, then its store
                mgrs = [vg.FontManager(False) for _ in locs]
                fids = [m.add_font_instance("Timed", data, loc) for m, loc in zip(mgrs, locs)]
                t0 = time.perf_counter()
                fonts = []
                for m, fid in zip(mgrs, fids):
                    d = m.command_font_desc(fid)
                    fonts.append(ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"]))
                t1 = time.perf_counter()
                for f in fonts:
                    f.free()
                # the descriptions for the device (views of the tables: no glyph is looked at)
                mgrs = [vg.FontManager(False) for _ in locs]
                descs = [m.gvar_font_desc(m.add_font_instance("Timed", data, loc)) for m, loc in zip(mgrs, locs)]
                t2 = time.perf_counter()
                fonts = [ctx.font_create_gvar(d) for d in descs]
                t3 = time.perf_counter()
                for f in fonts:
                    f.free()
                positions = [d["coords"] for d in descs]
                t4 = time.perf_counter()
                fonts, status, _ = ctx.fonts_create_gvar(descs[0], positions)
                t5 = time.perf_counter()
                assert status == [0] * n and all(f is not None for f in fonts)
                for f in fonts:
                    f.free()
                if run:      # (the first round pays for the context's scratch and the code objects' load)
                    host.append(t1 - t0), single.append(t3 - t2), batched.append(t5 - t4), passes.append(ctx.fonts_gvar_kernel_ms())
            ms = [statistics.median(p[i] for p in passes) for i in range(3)]
            h, s, b = med(host), med(single), med(batched)
            print(f"{kind:9s} N={n}  host {h:8.3f} ms ({h / n:7.3f} / instance)   single calls {s:8.3f} ms ({s / n:7.3f})   "
                  f"batched {b:8.3f} ms ({b / n:7.3f}; passes count {ms[0]:.3f}  deltas {ms[1]:.3f}  emit {ms[2]:.3f})   "
                  f"batched / host {b / h:5.2f}   batched / single {b / s:5.2f}")
    ctx.close()


if __name__ == "__main__":
    main()
