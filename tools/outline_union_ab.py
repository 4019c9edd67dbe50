"""What union outlines (rule U) cost: the union pass over a font id's full batch at the C ABI — count and emit
pass from HIP events, the whole vgsdf_batch_union call with its read-back and planning, the segments before and after —
and the raster over the union's list against the raster over the input list in the SAME session (switch off is the parent's
behaviour, so no second checkout is needed); then the façade's first render_glyphs of a fresh manager, switch off and on,
alternating.  Every run on a fresh context.
Inputs: Noto Sans Regular, and the 20-file Noto Sans id.
  python tools/outline_union_ab.py [--runs 20]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import NOTO, load_product, noto_files  # noqa: E402


def stats(v, unit=1e3):
    return f"best {min(v) * unit:9.3f} ms  median {statistics.median(v) * unit:9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--raster-iters", type=int, default=5)
    args = ap.parse_args()
    vg = load_product()
    inputs = [("Noto Sans Regular", [NOTO]), ("Noto Sans, 20 files, one font id", noto_files())]

    def abi_once(batch):
        """-> (count ms, emit ms, call seconds, raster ms over the input, over the union, segments in, out, states)"""
        ctx = vg.SdfContext(0)
        try:
            db = ctx.upload(batch)
            t0 = time.perf_counter()
            ub, state = db.union()
            call = time.perf_counter() - t0
            k = ctx.union_kernel_ms()
            db.time(1), ub.time(1)
            r_in = db.time(args.raster_iters) / args.raster_iters
            r_un = ub.time(args.raster_iters) / args.raster_iters
            n_in, n_out = db.stats()["n_segments"], ub.stats()["n_segments"]
            ub.free(), db.free()
        finally:
            ctx.close()
        return k[0], k[1], call, r_in, r_un, n_in, n_out, np.bincount(state, minlength=4)

    def facade_once(paths, union):
        mgr = vg.FontManager(True)
        mgr.set_union_outlines(union)
        mgr.add_font_with_name("Font", paths)
        r = vg.Renderer.new_precise(0)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        t = time.perf_counter() - t0
        s = mgr.union_stats()
        r.close()
        return t, s

    for name, paths in inputs:
        mgr = vg.FontManager(True)
        fid = mgr.add_font_with_name("Font", paths)
        hb = mgr.build_batch(fid)
        batch = hb.batch
        abi_once(batch), facade_once(paths, False), facade_once(paths, True)      # warm: code, allocator, clocks
        rows = [abi_once(batch) for _ in range(args.runs)]
        renders = {False: [], True: []}
        for _ in range(args.runs):
            for union in (False, True):
                renders[union].append(facade_once(paths, union))
        r0 = rows[0]
        seg_per = np.diff(batch.seg_off.astype(np.int64))
        print(f"\n{name}: {batch.n_glyphs} glyphs, largest {int(seg_per.max())} segments; segments {r0[5]} -> {r0[6]}; "
              f"states identity {r0[7][0]} rebuilt {r0[7][1]} over the limit {r0[7][2]} non-finite {r0[7][3]}; {args.runs} runs")
        print(f"  count pass            {stats([x[0] for x in rows], 1)}")
        print(f"  emit pass             {stats([x[1] for x in rows], 1)}")
        print(f"  vgsdf_batch_union     {stats([x[2] for x in rows])}   (both passes, the read-back of counts and descriptors, the work list, chunk boxes)")
        rest = [x[2] * 1e3 - x[0] - x[1] for x in rows]
        print(f"  the call less its passes  best {min(rest):9.3f} ms  median {statistics.median(rest):9.3f} ms   (the read-back of counts, states and "
              f"descriptors is NOT timed on its own: it is in this figure with the allocations, the host's work list and the chunk boxes)")
        print(f"  raster, input list    {stats([x[3] for x in rows], 1)}")
        print(f"  raster, union list    {stats([x[4] for x in rows], 1)}")
        for union, label in ((False, "switch off"), (True, "switch on ")):
            print(f"  façade, first render of a fresh manager, {label}: {stats([t for t, _ in renders[union]])}")
        print(f"  façade stats, switch on: {renders[True][0][1]}")
        hb.free()


if __name__ == "__main__":
    main()
