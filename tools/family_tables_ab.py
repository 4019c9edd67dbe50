"""A/B of the two ways to a resident family's table, the forms alternating in one process, every run on a fresh FontManager (so
the host's tables are built in the timed span: the first render of a font id is what is measured):
  (a) FontManager::family_table (a cmap lookup, an hmtx read and three f64 operations per code point) + vgsdf_family_create  [the baseline]
  (b) Face::family_tables per file (where the unicode subtables are; no lookup) + vgsdf_family_create_tables
at the C ABI, with the count and emit passes' own times from HIP events, and through the façade: the first render_glyphs of a
fresh manager with vg_manager_set_family_tables_on_device off and on (resident glyf fonts, resident families).
Inputs: Fira Sans, the 20-file Noto Sans id, and the 21 fixture fonts as 21 font ids.
  python tools/family_tables_ab.py [--runs 20]"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import FIRA, load_product, noto_files  # noqa: E402


def stats(v):
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    vg = load_product()
    from versatiles_glyphs_rs_amd import device as D, host as H
    L, HL = D.load_library(), H._L()
    ctx = vg.SdfContext(0)
    inputs = [("Fira Sans", [[FIRA]]), ("Noto Sans, 20 files, one font id", [noto_files()]),
              ("the 21 fixture fonts, 21 font ids", [[p] for p in [FIRA] + noto_files()])]

    def manager(ids):
        mgr = vg.FontManager(True)
        return mgr, [(mgr.add_font_with_name(f"Font {i}", paths), len(paths)) for i, paths in enumerate(ids)]

    def abi_once(ids, device):
        """-> (description seconds, create seconds, (count, emit) ms, entries, table bytes) summed over the font ids"""
        mgr, fids = manager(ids)
        t_desc = t_create = 0.0
        ms, entries, size = [0.0, 0.0], 0, 0
        for fid, n_files in fids:
            fonts = [ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"]) for d in (mgr.resident_font_desc(fid, k) for k in range(n_files))]
            handles = (C.c_void_p * n_files)(*[f._h for f in fonts])
            h = C.c_void_p()
            t0 = time.perf_counter()
            if device:
                recs = (D._CFaceTables * n_files)()
                for k in range(n_files):
                    assert HL.vg_manager_family_tables_desc(mgr._h, fid.encode(), k, C.cast(C.byref(recs[k]), C.POINTER(H._CFaceTables))) == 0
                d = D._CFamilyTablesDesc(n_files, C.cast(handles, C.c_void_p), C.cast(recs, C.c_void_p))
                t1 = time.perf_counter()
                rc = L.vgsdf_family_create_tables(ctx._h, C.byref(d), C.byref(h))
            else:
                v = H._CFamilyView()
                assert HL.vg_manager_family_desc(mgr._h, fid.encode(), C.byref(v)) == 0
                d = D._CFamilyDesc(n_files, C.cast(handles, C.c_void_p), v.n_entries, v.code_point, v.font_of, v.glyph_id, v.advance, v.scale, v.shift_x)
                t1 = time.perf_counter()
                rc = L.vgsdf_family_create(ctx._h, C.byref(d), C.byref(h))
            t2 = time.perf_counter()
            assert rc == 0, rc
            t_desc, t_create = t_desc + t1 - t0, t_create + t2 - t1
            if device:
                k = ctx.family_tables_kernel_ms()
                ms[0], ms[1] = ms[0] + k[0], ms[1] + k[1]
            entries += L.vgsdf_family_count(h, 0, 0xFFFF)
            size += L.vgsdf_family_device_bytes(h)
            L.vgsdf_family_free(ctx._h, h)
            for f in fonts:
                f.free()
        return t_desc, t_create, ms, entries, size

    def facade_once(ids, device):
        mgr, _ = manager(ids)
        mgr.set_resident_fonts(True)
        mgr.set_resident_families(True)
        mgr.set_family_tables_on_device(device)
        r = vg.Renderer.new_precise(0)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        t = time.perf_counter() - t0
        s = mgr.family_table_stats()
        assert s == {"built_on_device": len(ids) if device else 0, "fallbacks": 0}, s
        r.close()
        return t

    for name, ids in inputs:
        abi_once(ids, False), abi_once(ids, True), facade_once(ids, False), facade_once(ids, True)      # warm: code, allocator, clocks
        rows, renders = {False: [], True: []}, {False: [], True: []}
        for _ in range(args.runs):
            for device in (False, True):
                rows[device].append(abi_once(ids, device))
        for _ in range(args.runs):
            for device in (False, True):
                renders[device].append(facade_once(ids, device))
        assert rows[True][0][3:] == rows[False][0][3:]
        print(f"\n{name}: {rows[True][0][3]} entries, tables of {rows[True][0][4]} bytes on the device, {args.runs} runs each, alternating")
        for device, label in ((False, "(a) family_table + vgsdf_family_create        "), (True, "(b) family_tables + vgsdf_family_create_tables")):
            r = rows[device]
            print(f"  {label} description {stats([x[0] for x in r])} | create {stats([x[1] for x in r])} | both {stats([x[0] + x[1] for x in r])}")
        k = [x[2] for x in rows[True]]
        print(f"  passes of (b): count best {min(x[0] for x in k):.3f} ms median {statistics.median(x[0] for x in k):.3f} ms | "
              f"emit best {min(x[1] for x in k):.3f} ms median {statistics.median(x[1] for x in k):.3f} ms")
        for device, label in ((False, "switch off"), (True, "switch on ")):
            print(f"  façade, first render of a fresh manager, {label}: {stats(renders[device])}")
    ctx.close()


if __name__ == "__main__":
    main()
