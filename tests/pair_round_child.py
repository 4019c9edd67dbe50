"""Child process of tests/test_gpu_pair_rounds.py (not a test module): runs the sets of tests/pair_round_sets.py through the
counting instance of the MARGINS build (`make margins`; VGSDF_LIB must point at build/margins/libvgsdf.so) and prints ONE JSON
document: {set: {"pairs", "rounds", "wave_tile_chunks", "pool_overflows", "half_rounds", "left_after_phase1", "bytes" (hex)}}.
The last two counters are null when the library does not export vgsdf_margin_pair_round_counters.

It ends with a non-zero status at the first error (a HIP error surfaces as VgsdfError from the binding); nothing is started
on the GPU after that."""
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_product  # noqa: E402
import pair_round_sets as S  # noqa: E402

COUNT = 61  # vgsdf_set_variant id of the counting instance (csrc/sdf_margin_kernels.hip)


def run():
    vg = load_product()
    lib = vg.load_library()
    lib.vgsdf_margin_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lib.vgsdf_margin_counters.restype = ctypes.c_int
    more = getattr(lib, "vgsdf_margin_pair_round_counters", None)
    if more is not None:
        more.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
        more.restype = ctypes.c_int
    ctx = vg.SdfContext(0)
    ctx.set_variant(COUNT)
    doc = {}
    for name, gen in S.SETS.items():
        if lib.vgsdf_margin_counters(None, 1) != 0:
            raise RuntimeError("vgsdf_margin_counters: reset failed")
        out = ctx.render_batch(vg.make_batch(gen()))
        n = (ctypes.c_ulonglong * 9)()
        if lib.vgsdf_margin_counters(n, 0) != 0:
            raise RuntimeError("vgsdf_margin_counters: read failed")
        p = (ctypes.c_ulonglong * 2)()
        if more is not None and more(p) != 0:
            raise RuntimeError("vgsdf_margin_pair_round_counters: read failed")
        new = [int(v) for v in p] if more is not None else [None] * 2
        doc[name] = {"pairs": int(n[1]), "rounds": int(n[2]), "wave_tile_chunks": int(n[3]), "pool_overflows": int(n[6]),
                     "half_rounds": new[0], "left_after_phase1": new[1], "bytes": out.tobytes().hex()}
    ctx.close()
    return doc


if __name__ == "__main__":
    print(json.dumps(run()))
