"""A/B of the two ways to a CFF face's command store, warm, the forms alternating in one process:
  (a) Face::command_table() (the host reader interprets every glyph id twice) + vgsdf_font_create_commands   [the baseline]
  (b) Face::charstring_table() (INDEX offsets resolved, bodies copied)        + vgsdf_font_create_charstrings
with the count and emit kernels' own times from HIP events, on Fira Sans and Noto Sans Regular re-encoded as CFF and on a
synthetic CID-keyed face of about 60 000 glyph ids (Noto's charstrings repeated: the CJK case); then one façade render of
the CFF Noto face in mode 0, mode 1 with the switch off, and mode 1 with the switch on.
Every run takes a fresh FontManager, so both tables are built in the timed span (they are built once per face).
  python tools/charstrings_ab.py [--runs 20] [--skip-large]"""
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
from conftest import FIRA, NOTO, load_product  # noqa: E402
from fontTools.pens.t2CharStringPen import T2CharStringPen  # noqa: E402
from fontTools.ttLib import TTFont  # noqa: E402
import charstring_edge_programs as K  # noqa: E402
import test_cff_outlines as T  # noqa: E402


def as_cff(path, limit=None):
    src = TTFont(path)
    gs, order = src.getGlyphSet(), src.getGlyphOrder()[:limit]
    cs = {}
    for g in order:
        pen = T2CharStringPen(gs[g].width, gs)
        gs[g].draw(pen)
        cs[g] = pen.getCharString()
    cmap = {cp: g for cp, g in src.getBestCmap().items() if g in cs}
    return T._build(order, cmap, cs, {g: gs[g].width for g in order}, src["head"].unitsPerEm)


def cid_large(noto_cff, n_glyph_ids=60000):
    index = TTFont(io.BytesIO(noto_cff))["CFF "].cff.topDictIndex[0].CharStrings.charStringsIndex
    bodies = [index[g].bytecode for g in range(len(index))]
    glyphs = [bodies[g % len(bodies)] for g in range(n_glyph_ids)]
    return K.otf(K.cff_table(glyphs, [K.RET], [[K.RET], [K.RET, K.RET]], [g % 2 for g in range(n_glyph_ids)]), n_glyph_ids)


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
    HL.vg_manager_command_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    HL.vg_manager_charstring_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    ctx = vg.SdfContext(0)
    faces = [("Fira Sans as CFF", as_cff(FIRA)), ("Noto Sans Regular as CFF", as_cff(NOTO))]
    if not args.skip_large:
        faces.append(("synthetic CID-keyed, 60000 glyph ids", cid_large(faces[1][1])))

    def once(font, device):
        mgr = vg.FontManager(False)
        fid = mgr.add_font_data("Face", font).encode()
        h = C.c_void_p()
        t0 = time.perf_counter()
        if device:
            d = D._CFontCharstringsDesc()
            assert HL.vg_manager_charstring_font_desc(mgr._h, fid, 0, C.byref(d)) == 0
            t1 = time.perf_counter()
            rc = L.vgsdf_font_create_charstrings(ctx._h, C.byref(d), C.byref(h))
        else:
            d = D._CFontCmdsDesc()
            assert HL.vg_manager_command_font_desc(mgr._h, fid, 0, C.byref(d)) == 0
            t1 = time.perf_counter()
            rc = L.vgsdf_font_create_commands(ctx._h, C.byref(d), C.byref(h))
        t2 = time.perf_counter()
        assert rc == 0, rc
        size = L.vgsdf_font_device_bytes(h)
        L.vgsdf_font_free(ctx._h, h)
        return t1 - t0, t2 - t1, ctx.font_charstrings_kernel_ms() if device else (0.0, 0.0), d.n_glyph_ids, size

    for name, font in faces:
        once(font, False), once(font, True)                      # warm: code, allocator, clocks
        rows = {False: [], True: []}
        for _ in range(args.runs):
            for device in (False, True):
                rows[device].append(once(font, device))
        n, size = rows[True][0][3], rows[True][0][4]
        assert size == rows[False][0][4]
        print(f"\n{name}: {n} glyph ids, {len(font)} font bytes, store {size} bytes on the device, {args.runs} runs each, alternating")
        for device, label in ((False, "(a) command_table + create_commands   "), (True, "(b) charstring_table + create_charstrings")):
            r = rows[device]
            print(f"  {label} table {stats([x[0] for x in r])} | create {stats([x[1] for x in r])} | both {stats([x[0] + x[1] for x in r])}")
        k = [x[2] for x in rows[True]]
        print(f"  kernels of (b): count best {min(x[0] for x in k):.3f} ms median {statistics.median(x[0] for x in k):.3f} ms | "
              f"emit best {min(x[1] for x in k):.3f} ms median {statistics.median(x[1] for x in k):.3f} ms")

    # one façade render of the CFF Noto face, a fresh manager each (its tables unbuilt), one warm renderer
    font = faces[1][1]
    r = vg.Renderer.new_precise(0)
    configs = (("mode 0 (host reader on every render)", 0, False), ("mode 1, charstrings on the host", 1, False),
               ("mode 1, charstrings on the device", 1, True))

    def render(mode, on):
        mgr = vg.FontManager(True)
        mgr.set_resident_commands(mode)
        mgr.set_charstrings_on_device(on)
        mgr.add_font_data("Noto CFF", font)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        return time.perf_counter() - t0, w.files, mgr.charstring_stats()

    want = render(0, False)[1]
    times = {c[0]: [] for c in configs}
    for _ in range(max(5, args.runs // 2)):
        for label, mode, on in configs:
            t, files, s = render(mode, on)
            assert files == want and s["fonts_decoded"] == (1 if on else 0)
            times[label].append(t)
    print(f"\none façade render of Noto Sans Regular as CFF (first render of a fresh manager: the store is built in it), {len(times[configs[0][0]])} runs each")
    for label, _, _ in configs:
        print(f"  {label:40s} {stats(times[label])}")
    ctx.close()


if __name__ == "__main__":
    main()
