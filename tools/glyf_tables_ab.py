"""A/B of the three ways to the glyf-kind resident fonts of a font id, the forms alternating in one process, every run on a fresh
FontManager (so the host's table is built in the timed span: the first use of a face is what is measured):
  (a) Face::resident_table (every glyph id's composite tree walked, every simple entry copied) + vgsdf_font_create  [the baseline]
  (b) Face::font_tables (where loca and glyf are; no glyph looked at) + vgsdf_font_create_tables, one call per face
  (c) Face::font_tables of every face + ONE vgsdf_fonts_create_tables over all of them
at the C ABI, with the count and emit passes' own times from HIP events, and through the façade: the first render_glyphs of a
fresh manager with vg_manager_set_glyf_tables_on_device off, on, and on with vg_manager_set_glyf_tables_batched (resident glyf fonts).
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
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms  worst {max(v) * 1e3:8.3f} ms"


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

    def abi_once(files, form):
        """form 0 (a), 1 (b), 2 (c) -> (description seconds, create seconds, (count, emit) ms, leaves, font bytes) summed over the files"""
        mgr, fid = manager(files)
        t_desc = t_create = 0.0
        ms, leaves, size = [0.0, 0.0], 0, 0
        made = []
        if form == 2:
            n = len(files)
            descs, out, status = (D._CFontTablesDesc * n)(), (C.c_void_p * n)(), (C.c_int * n)()
            t0 = time.perf_counter()
            for k in range(n):
                assert HL.vg_manager_font_tables_desc(mgr._h, fid.encode(), k, C.byref(descs[k])) == 0
            t1 = time.perf_counter()
            rc = L.vgsdf_fonts_create_tables(ctx._h, descs, n, out, status)
            t2 = time.perf_counter()
            assert rc == 0 and not any(status) and all(out), (rc, list(status))
            t_desc, t_create, ms = t1 - t0, t2 - t1, list(ctx.fonts_tables_kernel_ms())
            made = [C.c_void_p(h) for h in out]
        else:
            for k in range(len(files)):
                h = C.c_void_p()
                t0 = time.perf_counter()
                if form == 1:
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
                if form == 1:
                    km = ctx.font_tables_kernel_ms()
                    ms[0], ms[1] = ms[0] + km[0], ms[1] + km[1]
                made.append(h)
        for h in made:                                                                 # (outside the timed spans)
            n_leaves = C.c_uint32()
            assert L.vgsdf_font_read(ctx._h, h, None, C.byref(n_leaves), None, None, None, None) == 0
            leaves += n_leaves.value
            size += L.vgsdf_font_device_bytes(h)
            L.vgsdf_font_free(ctx._h, h)
        return t_desc, t_create, ms, leaves, size

    def facade_once(files, form):
        mgr, _ = manager(files)
        mgr.set_resident_fonts(True)
        mgr.set_glyf_tables_on_device(form >= 1)
        mgr.set_glyf_tables_batched(form == 2)
        r = vg.Renderer.new_precise(0)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        t = time.perf_counter() - t0
        s, b = mgr.glyf_table_stats(), mgr.glyf_table_batch_stats()
        assert (s["built_on_device"], s["fallbacks"]) == (len(files) if form else 0, 0), s
        assert b == ({"calls": 1, "faces": len(files)} if form == 2 else {"calls": 0, "faces": 0}), b
        r.close()
        return t

    forms = (0, 1, 2)
    labels = {0: "(a) resident_table + vgsdf_font_create           ", 1: "(b) font_tables + vgsdf_font_create_tables, each  ",
              2: "(c) font_tables + ONE vgsdf_fonts_create_tables   "}
    for name, files, render in inputs:
        for form in forms:
            abi_once(files, form)                                                      # warm: code, allocator, clocks
        rows, renders = {f: [] for f in forms}, {f: [] for f in forms}
        for _ in range(args.runs):
            for form in forms:
                rows[form].append(abi_once(files, form))
        assert rows[0][0][3] == rows[1][0][3] == rows[2][0][3]
        print(f"\n{name}: {len(files)} file(s), {rows[1][0][3]} leaves, fonts of {rows[0][0][4]} (a) / {rows[1][0][4]} (b) / {rows[2][0][4]} (c) bytes on the device, "
              f"{args.runs} runs each, alternating")
        for form in forms:
            r = rows[form]
            print(f"  {labels[form]} description {stats([x[0] for x in r])} | create {stats([x[1] for x in r])} | both {stats([x[0] + x[1] for x in r])}")
        for form in (1, 2):
            k = [x[2] for x in rows[form]]
            print(f"  passes of ({'abc'[form]}), summed over its calls: count best {min(x[0] for x in k):.3f} ms median {statistics.median(x[0] for x in k):.3f} ms | "
                  f"emit + copy best {min(x[1] for x in k):.3f} ms median {statistics.median(x[1] for x in k):.3f} ms")
        if render:
            for form in forms:
                facade_once(files, form)
            for _ in range(args.runs):
                for form in forms:
                    renders[form].append(facade_once(files, form))
            for form, label in ((0, "switch off          "), (1, "tables on device    "), (2, "... and batched     ")):
                print(f"  façade, first render of a fresh manager, {label}: {stats(renders[form])}")
    ctx.close()


if __name__ == "__main__":
    main()
