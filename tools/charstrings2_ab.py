"""A/B of the two ways to a CFF2 face's command store, warm, the forms alternating in one process:
  (a) Face::command_table() (the host reader interprets every glyph id twice) + vgsdf_font_create_commands    [the baseline]
  (b) Face::charstring2_table() (INDEX offsets resolved, bodies copied, blend sets) + vgsdf_font_create_charstrings2
with the count and emit passes' own times from HIP events, on the variable Fira face of tests/test_cff2_outlines.py (two masters
merged by fontTools.varLib, 300 glyph ids) and on a synthetic face of 60 000 glyph ids that repeats its charstrings.  Beside
them, for the cost of the CFF2 stamping (513 operand slots, those past 48 in global memory; blends): the same outlines at the
default position as `CFF ` version 1 faces — the Regular master's charstrings, 300 and repeated to 60 000 — through
vgsdf_font_create_charstrings.  Every run takes a fresh FontManager, so the tables are built in the timed span.
  python tools/charstrings2_ab.py [--runs 20] [--skip-large]"""
import argparse
import ctypes as C
import io
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_product  # noqa: E402
from fontTools.ttLib import TTFont  # noqa: E402
import charstring2_edge_programs as K2  # noqa: E402
import charstring_edge_programs as K  # noqa: E402
from fira_cff_kit import fira_as_cff  # noqa: E402
from test_cff2_outlines import _variable_fira  # noqa: E402


def cff2_large(fira_cff2, n_glyph_ids):
    """the face's charstrings repeated, its subroutines, and sets of as many regions as its own (factor 0 at the default position,
    as the face's: one axis, every region peaks at its maximum)"""
    cff = TTFont(io.BytesIO(fira_cff2))["CFF2"].cff
    top = cff.topDictIndex[0]
    index = top.CharStrings.charStringsIndex
    bodies = [index[g].bytecode for g in range(len(index))]
    gsubrs = [s.bytecode for s in cff.GlobalSubrs]
    lsubrs = [s.bytecode for s in next((fd.Private.Subrs for fd in top.FDArray if getattr(fd.Private, "Subrs", None)), [])]
    sets = [[1] * len(d.VarRegionIndex) for d in top.VarStore.otVarStore.VarData]
    glyphs = [bodies[g % len(bodies)] for g in range(n_glyph_ids)]
    return K2.otf(K2.cff2_table(glyphs, gsubrs, lsubrs, sets), n_glyph_ids)


def cff_large(fira_cff, n_glyph_ids):
    cff = TTFont(io.BytesIO(fira_cff))["CFF "].cff
    top = cff.topDictIndex[0]
    index = top.CharStrings.charStringsIndex
    bodies = [index[g].bytecode for g in range(len(index))]
    gsubrs = [s.bytecode for s in cff.GlobalSubrs]
    lsubrs = [s.bytecode for s in getattr(top.Private, "Subrs", [])]
    return K.otf(K.cff_table([bodies[g % len(bodies)] for g in range(n_glyph_ids)], gsubrs, [lsubrs]), n_glyph_ids)


def stats(v):
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    vg = load_product()
    from versatiles_glyphs_rs_amd import device as D, host as H
    L, HL = D.load_library(), H._L()
    for f in ("vg_manager_command_font_desc", "vg_manager_charstring_font_desc", "vg_manager_charstring2_font_desc"):
        getattr(HL, f).argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    ctx = vg.SdfContext(0)
    fira2, fira1 = _variable_fira(), fira_as_cff(300)
    faces = [("variable Fira, CFF2", fira2, True), ("the same outlines (Regular master), CFF version 1", fira1, False)]
    if not args.skip_large:
        faces += [("variable Fira's charstrings repeated, CFF2, 60000 glyph ids", cff2_large(fira2, 60000), True),
                  ("the Regular master's charstrings repeated, CFF version 1, 60000 glyph ids", cff_large(fira1, 60000), False)]

    def once(font, device, cff2):
        mgr = vg.FontManager(False)
        fid = mgr.add_font_data("Face", font).encode()
        h = C.c_void_p()
        t0 = time.perf_counter()
        if device and cff2:
            d = D._CFontCharstrings2Desc()
            assert HL.vg_manager_charstring2_font_desc(mgr._h, fid, 0, C.byref(d)) == 0
            t1 = time.perf_counter()
            rc = L.vgsdf_font_create_charstrings2(ctx._h, C.byref(d), C.byref(h))
            n = d.charstrings.n_glyph_ids
        elif device:
            d = D._CFontCharstringsDesc()
            assert HL.vg_manager_charstring_font_desc(mgr._h, fid, 0, C.byref(d)) == 0
            t1 = time.perf_counter()
            rc = L.vgsdf_font_create_charstrings(ctx._h, C.byref(d), C.byref(h))
            n = d.n_glyph_ids
        else:
            d = D._CFontCmdsDesc()
            assert HL.vg_manager_command_font_desc(mgr._h, fid, 0, C.byref(d)) == 0
            t1 = time.perf_counter()
            rc = L.vgsdf_font_create_commands(ctx._h, C.byref(d), C.byref(h))
            n = d.n_glyph_ids
        t2 = time.perf_counter()
        assert rc == 0, rc
        size = L.vgsdf_font_device_bytes(h)
        L.vgsdf_font_free(ctx._h, h)
        return t1 - t0, t2 - t1, ctx.font_charstrings_kernel_ms() if device else (0.0, 0.0), n, size

    for name, font, cff2 in faces:
        once(font, False, cff2), once(font, True, cff2)                      # warm: code, allocator, clocks
        rows = {False: [], True: []}
        for _ in range(args.runs):
            for device in (False, True):
                rows[device].append(once(font, device, cff2))
        n, size = rows[True][0][3], rows[True][0][4]
        assert size == rows[False][0][4]
        print(f"\n{name}: {n} glyph ids, {len(font)} font bytes, store {size} bytes on the device, {args.runs} runs each, alternating")
        b = "(b) charstring2_table + create_charstrings2" if cff2 else "(b) charstring_table + create_charstrings  "
        for device, label in ((False, "(a) command_table + create_commands       "), (True, b)):
            r = rows[device]
            print(f"  {label} table {stats([x[0] for x in r])} | create {stats([x[1] for x in r])} | both {stats([x[0] + x[1] for x in r])}")
        k = [x[2] for x in rows[True]]
        print(f"  passes of (b): count best {min(x[0] for x in k):.3f} ms median {statistics.median(x[0] for x in k):.3f} ms | "
              f"emit best {min(x[1] for x in k):.3f} ms median {statistics.median(x[1] for x in k):.3f} ms")
    ctx.close()


if __name__ == "__main__":
    main()
