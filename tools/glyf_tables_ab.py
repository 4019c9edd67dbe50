"""A/B of the two ways to a glyf-kind resident font, the forms alternating in one process, every run on a fresh FontManager (so
the host's table is built in the timed span: the first use of a face is what is measured):
  (a) Face::resident_table (every glyph id's composite tree walked, every simple entry copied) + vgsdf_font_create  [the baseline]
  (b) Face::font_tables (where loca and glyf are; no glyph looked at) + vgsdf_font_create_tables
at the C ABI, with the count and emit passes' own times from HIP events, and through the façade: the first render_glyphs of a
fresh manager with vg_manager_set_glyf_tables_on_device off and on (resident glyf fonts).
Inputs: Fira Sans, Noto Sans Regular, the 20 Noto files, and Noto Sans Regular's glyphs repeated to 60 000 glyph ids (C ABI only).
  python tools/glyf_tables_ab.py [--runs 20]"""
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
from conftest import FIRA, NOTO, load_product, noto_files  # noqa: E402


def stats(v):
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms"


def repeated(path, n_glyphs):
    """the font with its glyph entries repeated until it has n_glyphs glyph ids (loca long; composites keep naming the first copy)"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    f = TTFont(str(path), recalcBBoxes=False, recalcTimestamp=False)
    glyf, loca = f.reader["glyf"], f.reader["loca"]
    long, n = f["head"].indexToLocFormat, f["maxp"].numGlyphs
    size = 4 if long else 2
    offs = [int.from_bytes(loca[size * i:size * i + size], "big") * (1 if long else 2) for i in range(n + 1)]
    copies = (n_glyphs + n - 1) // n
    new = [(i // n) * len(glyf) + offs[i % n] for i in range(n_glyphs)]
    new.append((((n_glyphs - 1) // n) * len(glyf)) + offs[(n_glyphs - 1) % n + 1])
    raw = {tag: bytearray(f.reader[tag]) for tag in ("head", "maxp", "hhea")}
    raw["head"][50:52] = (1).to_bytes(2, "big")
    raw["maxp"][4:6] = n_glyphs.to_bytes(2, "big")
    raw["glyf"] = glyf * copies
    raw["loca"] = b"".join(o.to_bytes(4, "big") for o in new)
    for tag, data in raw.items():
        t = DefaultTable(tag)
        t.data = bytes(data)
        f[tag] = t
    buf = io.BytesIO()
    f.save(buf)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    vg = load_product()
    from versatiles_glyphs_rs_amd import device as D, host as H
    L, HL = D.load_library(), H._L()
    HL.vg_manager_resident_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    HL.vg_manager_font_tables_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    ctx = vg.SdfContext(0)
    big = repeated(NOTO, 60000)
    inputs = [("Fira Sans", [FIRA], True), ("Noto Sans Regular", [NOTO], True), ("Noto Sans, 20 files", noto_files(), True),
              ("Noto Sans Regular repeated to 60 000 glyph ids", [big], False)]

    def manager(files):
        mgr = vg.FontManager(True)
        if isinstance(files[0], bytes):
            return mgr, mgr.add_font_data("Font", files[0])
        return mgr, mgr.add_font_with_name("Font", files)

    def abi_once(files, device):
        """-> (description seconds, create seconds, (count, emit) ms, leaves, font bytes) summed over the files"""
        mgr, fid = manager(files)
        t_desc = t_create = 0.0
        ms, leaves, size = [0.0, 0.0], 0, 0
        for k in range(len(files)):
            h, n_leaves = C.c_void_p(), C.c_uint32()
            t0 = time.perf_counter()
            if device:
                d = D._CFontTablesDesc()
                assert HL.vg_manager_font_tables_desc(mgr._h, fid.encode(), k, C.byref(d)) == 0
                t1 = time.perf_counter()
                rc = L.vgsdf_font_create_tables(ctx._h, C.byref(d), C.byref(h))
            else:
                d = D._CFontDesc()
                assert HL.vg_manager_resident_font_desc(mgr._h, fid.encode(), k, C.byref(d)) == 0
                t1 = time.perf_counter()
                rc = L.vgsdf_font_create(ctx._h, C.byref(d), C.byref(h))
            t2 = time.perf_counter()
            assert rc == 0, rc
            t_desc, t_create = t_desc + t1 - t0, t_create + t2 - t1
            if device:
                km = ctx.font_tables_kernel_ms()
                ms[0], ms[1] = ms[0] + km[0], ms[1] + km[1]
            assert L.vgsdf_font_read(ctx._h, h, None, C.byref(n_leaves), None, None, None, None) == 0
            leaves += n_leaves.value
            size += L.vgsdf_font_device_bytes(h)
            L.vgsdf_font_free(ctx._h, h)
        return t_desc, t_create, ms, leaves, size

    def facade_once(files, device):
        mgr, _ = manager(files)
        mgr.set_resident_fonts(True)
        mgr.set_glyf_tables_on_device(device)
        r = vg.Renderer.new_precise(0)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        t = time.perf_counter() - t0
        s = mgr.glyf_table_stats()
        assert (s["built_on_device"], s["fallbacks"]) == (len(files) if device else 0, 0), s
        r.close()
        return t

    for name, files, render in inputs:
        abi_once(files, False), abi_once(files, True)                                  # warm: code, allocator, clocks
        rows, renders = {False: [], True: []}, {False: [], True: []}
        for _ in range(args.runs):
            for device in (False, True):
                rows[device].append(abi_once(files, device))
        assert rows[True][0][3] == rows[False][0][3]
        print(f"\n{name}: {rows[True][0][3]} leaves, fonts of {rows[False][0][4]} (a) / {rows[True][0][4]} (b) bytes on the device, {args.runs} runs each, alternating")
        for device, label in ((False, "(a) resident_table + vgsdf_font_create    "), (True, "(b) font_tables + vgsdf_font_create_tables")):
            r = rows[device]
            print(f"  {label} description {stats([x[0] for x in r])} | create {stats([x[1] for x in r])} | both {stats([x[0] + x[1] for x in r])}")
        k = [x[2] for x in rows[True]]
        print(f"  passes of (b): count best {min(x[0] for x in k):.3f} ms median {statistics.median(x[0] for x in k):.3f} ms | "
              f"emit + copy best {min(x[1] for x in k):.3f} ms median {statistics.median(x[1] for x in k):.3f} ms")
        if render:
            facade_once(files, False), facade_once(files, True)
            for _ in range(args.runs):
                for device in (False, True):
                    renders[device].append(facade_once(files, device))
            for device, label in ((False, "switch off"), (True, "switch on ")):
                print(f"  façade, first render of a fresh manager, {label}: {stats(renders[device])}")
    ctx.close()


if __name__ == "__main__":
    main()
