"""Timings of the family tables of N instances of ONE variable file, medians of --runs, three sides alternating in one process,
every round on a fresh FontManager (so the host's tables are built in the timed span); the stores are made before the clock starts:
  host     N x ( FontManager.family_desc: the reader's table  +  vgsdf_family_create of it )
  single   N x vgsdf_family_create_tables_gvar of the face's cmap, hmtx and HVAR record or loca, glyf and gvar at the position
  batched  one vgsdf_families_create_tables over the N positions (the whole call, and its phantom / count / emit passes by HIP events)
Inputs: the 315-glyph fixtures of tests/gvar_instances_kit.py (sheared second master, pure-scale second master, two axes) WITH their
HVAR and with HVAR removed (the advances then follow gvar's phantom points, vg_manager_set_gvar_advances), at N = 1, 3, 9 positions
spread over the weight axis (two axes: weight and width together).  Needs a device.
  python tools/family_batch_ab.py [--runs 21]"""
import argparse
import io
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
ENTRY_KEYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")


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


def without_hvar(data):
    from fontTools.ttLib import TTFont
    f = TTFont(io.BytesIO(data))
    del f["HVAR"]
    out = io.BytesIO()
    f.save(out)
    return out.getvalue()


def placed(vg, data, locs):
    """a fresh manager with a font id per position"""
    mgr = vg.FontManager(False)
    mgr.set_gvar_advances(True)
    return mgr, [mgr.add_font_instance(f"Timed {k}", data, loc) for k, loc in enumerate(locs)]


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
        for hvar in (True, False):
            data = G.variable_glyf_fira(kind) if hvar else without_hvar(G.variable_glyf_fira(kind))
            for n in (1, 3, 9):
                locs = locations(kind, n)
                mgr, fids = placed(vg, data, locs)
                positions = [mgr.gvar_font_desc(fid)["coords"] for fid in fids]
                stores, status, _ = ctx.fonts_create_gvar(mgr.gvar_font_desc(fids[0]), positions)
                assert status == [0] * n
                host, single, batched, passes = [], [], [], []
                for run in range(args.runs + 1):
                    m, ids = placed(vg, data, locs)
                    t0 = time.perf_counter()
                    fams = []
                    for fid, store in zip(ids, stores):
                        e = m.family_desc(fid)
                        fams.append(ctx.family_create([store], *[e[k] for k in ENTRY_KEYS]))
                    t1 = time.perf_counter()
                    want = [ctx.family_read(f)["advance"].tobytes() for f in fams]
                    for f in fams:
                        f.free()
                    # the descriptions for the device (views of the tables: no code point is looked up)
                    m, ids = placed(vg, data, locs)
                    tables = [m.family_tables_desc(fid, 0) for fid in ids]
                    var = [m.family_variation_desc(fid, 0) for fid in ids]
                    gvar = [m.family_gvar_desc(fid, 0) for fid in ids]
                    assert all(bool(v) == hvar for v in var) and all((g is None) == hvar for g in gvar)
                    t2 = time.perf_counter()
                    fams = [ctx.family_create_tables_gvar([s], [t], [v], [g]) for s, t, v, g in zip(stores, tables, var, gvar)]
                    t3 = time.perf_counter()
                    for f in fams:
                        f.free()
                    t4 = time.perf_counter()
                    fams, status = ctx.families_create_tables(stores, tables[0], var if hvar else None, gvar[0], positions if not hvar else None)
                    t5 = time.perf_counter()
                    assert status == [0] * n and [ctx.family_read(f)["advance"].tobytes() for f in fams] == want
                    for f in fams:
                        f.free()
                    if run:      # (the first round pays for the context's array and the code objects' load)
                        host.append(t1 - t0), single.append(t3 - t2), batched.append(t5 - t4), passes.append(ctx.families_tables_kernel_ms())
                ms = [statistics.median(p[i] for p in passes) for i in range(3)]
                h, s, b = med(host), med(single), med(batched)
                print(f"{kind:9s} {'HVAR   ' if hvar else 'no HVAR'} N={n}  host {h:7.3f} ms ({h / n:6.3f} / instance)   single calls {s:7.3f} ms "
                      f"({s / n:6.3f})   batched {b:7.3f} ms ({b / n:6.3f}; passes phantom {ms[0]:.3f}  count {ms[1]:.3f}  emit {ms[2]:.3f})   "
                      f"batched / host {b / h:5.2f}   batched / single {b / s:5.2f}", flush=True)
                for f in stores:
                    f.free()
    ctx.close()


if __name__ == "__main__":
    main()
