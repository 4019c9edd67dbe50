"""Child process of tests/test_gpu_sweep_shapes.py (not a test module): runs the round-count sets of tests/sweep_shapes_sets.py
through the counting instance of the MARGINS build (`make margins`; VGSDF_LIB must point at build/margins/libvgsdf.so) and
prints ONE JSON document: {set: {"pairs", "rounds", "wave_tile_chunks", "pool_overflows", "bytes" (hex)}}.

It ends with a non-zero status at the first error (a HIP error surfaces as VgsdfError from the binding); nothing is started
on the GPU after that."""
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_product  # noqa: E402
import sweep_shapes_sets as S  # noqa: E402

COUNT = 61  # vgsdf_set_variant id of the counting instance (csrc/sdf_margin_kernels.hip)


def run():
    vg = load_product()
    lib = vg.load_library()
    lib.vgsdf_margin_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lib.vgsdf_margin_counters.restype = ctypes.c_int
    ctx = vg.SdfContext(0)
    ctx.set_variant(COUNT)
    doc = {}
    for name, gen in S.ROUND_SETS.items():
        if lib.vgsdf_margin_counters(None, 1) != 0:
            raise RuntimeError("vgsdf_margin_counters: reset failed")
        out = ctx.render_batch(vg.make_batch(gen()))
        n = (ctypes.c_ulonglong * 9)()
        if lib.vgsdf_margin_counters(n, 0) != 0:
            raise RuntimeError("vgsdf_margin_counters: read failed")
        doc[name] = {"pairs": int(n[1]), "rounds": int(n[2]), "wave_tile_chunks": int(n[3]), "pool_overflows": int(n[6]),
                     "bytes": out.tobytes().hex()}
    ctx.close()
    return doc


if __name__ == "__main__":
    print(json.dumps(run()))
