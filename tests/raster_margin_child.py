"""Child process of tests/test_gpu_raster_margins.py (not a test module): runs every input set through the instances of
the MARGINS build (`make margins`; VGSDF_LIB must point at build/margins/libvgsdf.so) and prints ONE JSON document:

    {"diff": {instance: {set: bytes that differ from the oracle}}, "counters": {set: {counter: value}}, "pixels": {set: n}}

It ends with a non-zero status at the first error (a HIP error surfaces as VgsdfError from the binding); nothing is
started on the GPU after that.  `python tests/raster_margin_child.py --table` prints the matrix as text instead
(profiles/raster_margin_kills.txt)."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_product  # noqa: E402
import raster_margin_sets as S  # noqa: E402

# vgsdf_set_variant ids of csrc/sdf_margin_kernels.hip
BASE, COUNT = 60, 61
WEAKENED = {"a_dl0": 62, "b_e0": 63, "c_tk_f1": 64, "d_rg0": 65, "e_sat3": 66, "f_far20": 67, "g_sane": 68, "h_bounded": 69,
            "i_box_r0": 70, "j_box_band": 71, "k_e64_0": 72, "k_mabs0_0": 73, "l_infl_pad": 74}
GRADED = {"e/2": 75, "e/4": 76, "e/8": 77, "dl/2": 78, "dl/4": 79, "dl/8": 80, "r_g/2": 81, "r_g/4": 82, "r_g/8": 83}
COUNTERS = ("waves", "pairs", "rounds", "wave_tile_chunks", "waves_undecided", "undecided_lanes", "pool_overflows",
            "waves_pooled_exact", "waves_per_lane_exact")


def run():
    from oracle import oracle as O
    vg = load_product()
    lib = vg.load_library()
    lib.vgsdf_margin_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lib.vgsdf_margin_counters.restype = ctypes.c_int
    ctx = vg.SdfContext(0)
    sets = dict(S.new_sets())
    sets.update({s.name: s for s in S.old_sets()})
    instances = {"product_0": 0, "base": BASE, **WEAKENED, **GRADED}
    doc = {"diff": {k: {} for k in instances}, "counters": {}, "pixels": {}}
    for name, s in sets.items():
        batch = vg.make_batch(s.glyphs)
        want, _ = O.sdf_render_batch(batch, O.BRUTE, 8)
        doc["pixels"][name] = int(want.size)
        for inst, variant in instances.items():
            ctx.set_variant(variant)
            doc["diff"][inst][name] = int((ctx.render_batch(batch) != want).sum())
        ctx.set_variant(COUNT)
        if lib.vgsdf_margin_counters(None, 1) != 0:
            raise RuntimeError("vgsdf_margin_counters: reset failed")
        got = ctx.render_batch(batch)
        c = (ctypes.c_ulonglong * 9)()
        if lib.vgsdf_margin_counters(c, 0) != 0:
            raise RuntimeError("vgsdf_margin_counters: read failed")
        doc["counters"][name] = dict(zip(COUNTERS, (int(v) for v in c)))
        doc["diff"].setdefault("count", {})[name] = int((got != want).sum())
    ctx.set_variant(0)
    ctx.close()
    return doc


def table(doc):
    names = list(doc["pixels"])
    out = ["bytes that differ from the oracle (BRUTE), instance x set; '.' = 0", ""]
    for i, n in enumerate(names):
        out.append(f"  [{i:2d}] {n:24s} {doc['pixels'][n]:7d} px")
    out.append("")
    out.append(f"{'instance':12s}" + "".join(f"{i:>6d}" for i in range(len(names))))
    for inst, row in doc["diff"].items():
        out.append(f"{inst:12s}" + "".join(f"{row[n] if row[n] else '.':>6}" for n in names))
    out += ["", "counters of the counting instance, per set", "", f"{'set':24s}" + "".join(f"{c[:12]:>13s}" for c in COUNTERS[3:])]
    for n in names:
        out.append(f"{n:24s}" + "".join(f"{doc['counters'][n][c]:>13d}" for c in COUNTERS[3:]))
    return "\n".join(out)


if __name__ == "__main__":
    d = run()
    print(table(d) if "--table" in sys.argv[1:] else json.dumps(d))
