"""Timings of a family's table for a placed glyf face WITHOUT `HVAR` whose advances follow gvar's phantom points (rule G7 of
csrc/host/ttf_face.hpp; vg_manager_set_gvar_advances), medians of --runs, every run on a fresh FontManager (so the host's table
is built in the timed span), alternating between
    host    FontManager.family_desc (the reader's table: cmap enumeration, and per glyph id the streaming walk of its tuples for
            the advance) plus vgsdf_family_create of it, and
    device  vgsdf_family_create_tables_gvar of the face's cmap and hmtx and its loca, glyf and gvar (the whole call; its phantom
            pass and its count / emit passes by HIP events),
and, for scale, the same two for the SAME file with its HVAR (vgsdf_family_create_tables_var: no phantom pass) and the phantom
pass alone (vgsdf_gvar_advance_deltas).  Needs a device.
Inputs: the 315-glyph fixtures of tests/phantom_advances_kit.py (sheared second master, pure-scale second master, two axes).
  python tools/gvar_advances_ab.py [--runs 11]"""
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
    ap.add_argument("--runs", type=int, default=11)
    args = ap.parse_args()
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE / "tests"))
    from conftest import load_product
    vg = load_product()
    import gvar_instances_kit as G
    import phantom_advances_kit as P
    ctx = vg.SdfContext(0)
    keys = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")

    def placed(data, loc):
        mgr = vg.FontManager(False)
        mgr.set_gvar_advances(True)
        return mgr, mgr.add_font_instance("Timed", data, loc)

    for kind, loc in (("shear", {"wght": 650}), ("scale", {"wght": 650}), ("two_axes", G.EXACT_TWO_AXES[1])):
        for label, data in (("no HVAR", P.without_hvar(kind)), ("HVAR", G.variable_glyf_fira(kind))):
            mgr, fid = placed(data, loc)
            cmds = mgr.command_font_desc(fid)
            store = ctx.font_create_commands(cmds["cmd_off"], cmds["dat_off"], cmds["kinds"], cmds["coords"])
            table, upload, device, phantom, passes, alone, n = [], [], [], [], [], [], 0
            for run in range(args.runs + 1):
                mgr, fid = placed(data, loc)
                t0 = time.perf_counter()
                host = mgr.family_desc(fid)
                t1 = time.perf_counter()
                f = ctx.family_create([store], *[host[k] for k in keys])
                t2 = time.perf_counter()
                f.free()
                mgr, fid = placed(data, loc)
                tables, var, gvar = mgr.family_tables_desc(fid, 0), mgr.family_variation_desc(fid, 0), mgr.family_gvar_desc(fid, 0)
                assert (gvar is not None) == (label == "no HVAR")
                t3 = time.perf_counter()
                f = ctx.family_create_tables_gvar([store], [tables], [var], [gvar])
                t4 = time.perf_counter()
                got = ctx.family_read(f)
                f.free()
                assert got["advance"].tobytes() == host["advance"].tobytes()
                if run:          # (the first round pays for the context's buffers and the code objects' load)
                    table.append(t1 - t0), upload.append(t2 - t1), device.append(t4 - t3)
                    phantom.append(ctx.gvar_advance_kernel_ms()), passes.append(ctx.family_tables_kernel_ms())
                    if gvar is not None:
                        ctx.gvar_advance_deltas(gvar)
                        alone.append(ctx.gvar_advance_kernel_ms())
                n = len(host["code_point"])
            ms = [statistics.median(p[i] for p in passes) for i in range(2)]
            print(f"{kind:9s} {label:8s} {n:5d} entries   host: table {stats(table)}  + family_create {stats(upload)}")
            print(f"{'':9s} {'':8s} {'':5s}           device: create_tables_gvar {stats(device)}  (passes, median: phantom "
                  f"{statistics.median(phantom):.3f}  count {ms[0]:.3f}  emit {ms[1]:.3f} ms)")
            if alone:
                print(f"{'':9s} {'':8s} {'':5s}           the phantom pass alone (vgsdf_gvar_advance_deltas): median {statistics.median(alone):.3f} ms")
            store.free()
    ctx.close()


if __name__ == "__main__":
    main()
