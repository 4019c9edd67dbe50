"""Child process of tests/test_gpu_stage_filters.py (not a test module): runs the sets of tests/stage_filter_sets.py through
the instances of the MARGINS build that concern the stage's f32 decision (`make margins`; VGSDF_LIB must point at
build/margins/libvgsdf.so) and prints ONE JSON document:

    {"diff": {instance: {set: bytes that differ from the oracle}}, "counters": {set: {counter: value}}, "pixels": {set: n}}

It ends with a non-zero status at the first error (a HIP error surfaces as VgsdfError from the binding); nothing is started
on the GPU after that.  `python tests/stage_filter_child.py --table` prints the document as text instead."""
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_product  # noqa: E402
import stage_filter_sets as S  # noqa: E402

# vgsdf_set_variant ids of csrc/sdf_margin_kernels.hip
INSTANCES = {"product_0": 0, "base": 60, "count": 61, "m_row_e0": 84}
COUNTERS = ("row_fallback_waves",)


def run():
    from oracle import oracle as O
    vg = load_product()
    lib = vg.load_library()
    lib.vgsdf_margin_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lib.vgsdf_margin_counters.restype = ctypes.c_int
    lib.vgsdf_margin_stage_filter_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    lib.vgsdf_margin_stage_filter_counters.restype = ctypes.c_int
    ctx = vg.SdfContext(0)
    doc = {"diff": {k: {} for k in INSTANCES}, "counters": {}, "pixels": {}}
    for name, glyphs in S.sets().items():
        batch = vg.make_batch(glyphs)
        want, _ = O.sdf_render_batch(batch, O.BRUTE, 8)
        doc["pixels"][name] = int(want.size)
        for inst, variant in INSTANCES.items():
            ctx.set_variant(variant)
            if inst == "count" and lib.vgsdf_margin_counters(None, 1) != 0:
                raise RuntimeError("vgsdf_margin_counters: reset failed")
            doc["diff"][inst][name] = int((ctx.render_batch(batch) != want).sum())
            if inst == "count":
                c = (ctypes.c_ulonglong * 1)()
                if lib.vgsdf_margin_stage_filter_counters(c) != 0:
                    raise RuntimeError("vgsdf_margin_stage_filter_counters: read failed")
                doc["counters"][name] = dict(zip(COUNTERS, (int(v) for v in c)))
    ctx.set_variant(0)
    ctx.close()
    return doc


def table(doc):
    names = list(doc["pixels"])
    out = ["bytes that differ from the oracle (BRUTE), instance x set; '.' = 0", ""]
    out.append(f"{'instance':12s}" + "".join(f"{n[:10]:>11s}" for n in names))
    for inst, row in doc["diff"].items():
        out.append(f"{inst:12s}" + "".join(f"{row[n] if row[n] else '.':>11}" for n in names))
    out += ["", "counters of the counting instance, per set", ""]
    for c in COUNTERS:
        out.append(f"{c:20s}" + "".join(f"{doc['counters'][n][c]:>11d}" for n in names))
    return "\n".join(out)


if __name__ == "__main__":
    d = run()
    print(table(d) if "--table" in sys.argv[1:] else json.dumps(d))
