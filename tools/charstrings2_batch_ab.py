"""Timings of the command stores of N instances of ONE variable CFF2 file, medians of --runs, three sides alternating in one
process, every round on fresh FontManagers and, per side, a fresh device context (so each side pays once per round for the
context's workspace of the operand stack, as a first build in a process does):
  host     N x ( Face::command_table() through vg_manager_command_font_desc  +  vgsdf_font_create_commands of it )
  single   N x vgsdf_font_create_charstrings2 of the face's charstrings with the instance's factors
  batched  one vgsdf_fonts_create_charstrings2 over the N positions
with the count / emit passes of the last single call and of the batched call by HIP events.  The descriptions of the device's
sides (views of the INDEXes, no glyph is interpreted) are built outside the timed span, as tools/gvar_batch_ab.py does.
Inputs: the variable Fira face of tests/variable_instances_kit.py, 300 glyph ids, with one and two axes, and (unless --skip-large)
the one-axis face's charstrings repeated to 60 000 glyph ids, at N = 1, 3, 9 positions spread over the axes.
Then the façade: vg_renderer_preload_fonts and the first vg_manager_render_glyphs of the nine-instance file of
tests/charstring2_batch_kit.py with vg_manager_set_charstrings_on_device(m, 2), vg_manager_set_charstrings_batched off and on,
fresh manager and renderer every round.  Needs a device.
  python tools/charstrings2_batch_ab.py [--runs 21] [--skip-large]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def locations(two_axes, n):
    """n positions off the default, evenly spread"""
    out = []
    for k in range(n):
        t = (k + 1) / n
        loc = {"wght": 400 + 500 * t}
        if two_axes:
            loc["wdth"] = 100 + 100 * t
        out.append(loc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE / "tools"))
    sys.path.insert(0, str(HERE / "tests"))
    from conftest import load_product
    vg = load_product()
    import charstring2_batch_kit as B
    import variable_instances_kit as V
    med = lambda v: statistics.median(v) * 1e3  # noqa: E731
    faces = [("fira_1_axis", V.variable_fira(300), False), ("fira_2_axes", V.variable_fira(300, two_axes=True), True)]
    if not args.skip_large:
        from charstrings2_ab import cff2_large
        faces.append(("fira_x_60000", cff2_large(V.variable_fira(300), 60000), False))
    for kind, data, two_axes in faces:
        for n in (1, 3, 9):
            locs = locations(two_axes, n)
            host, single, batched, single_ms, batched_ms = [], [], [], [], []
            for run in range(args.runs + 1):
                # host: the table of every instance, then its store
                ctx = vg.SdfContext(0)
                mgrs = [vg.FontManager(False) for _ in locs]
                fids = [m.add_font_instance("Timed", data, loc) for m, loc in zip(mgrs, locs)]
                t0 = time.perf_counter()
                fonts = []
                for m, fid in zip(mgrs, fids):
                    d = m.command_font_desc(fid)
                    fonts.append(ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"]))
                t1 = time.perf_counter()
                sizes = [f.device_bytes for f in fonts]
                for f in fonts:
                    f.free()
                ctx.close()
                # the descriptions for the device
                mgrs = [vg.FontManager(False) for _ in locs]
                descs = [m.charstring2_font_desc(m.add_font_instance("Timed", data, loc)) for m, loc in zip(mgrs, locs)]
                ctx = vg.SdfContext(0)
                t2 = time.perf_counter()
                fonts = [ctx.font_create_charstrings2(d) for d in descs]
                t3 = time.perf_counter()
                assert [f.device_bytes for f in fonts] == sizes
                for f in fonts:
                    f.free()
                s_ms = ctx.font_charstrings_kernel_ms()
                ctx.close()
                positions = [d["factors"] for d in descs]
                ctx = vg.SdfContext(0)
                t4 = time.perf_counter()
                fonts, status, _ = ctx.fonts_create_charstrings2(descs[0], positions)
                t5 = time.perf_counter()
                assert status == [0] * n and [f.device_bytes for f in fonts] == sizes
                for f in fonts:
                    f.free()
                b_ms = ctx.fonts_charstrings2_kernel_ms()
                ctx.close()
                if run:      # (the first round pays for the code objects' load)
                    host.append(t1 - t0), single.append(t3 - t2), batched.append(t5 - t4), single_ms.append(s_ms), batched_ms.append(b_ms)
            sm = [statistics.median(p[i] for p in single_ms) for i in range(2)]
            bm = [statistics.median(p[i] for p in batched_ms) for i in range(2)]
            h, s, b = med(host), med(single), med(batched)
            print(f"{kind:13s} N={n}  host {h:8.3f} ms ({h / n:7.3f} / instance)   single calls {s:8.3f} ms ({s / n:7.3f}; passes of one call "
                  f"count {sm[0]:.3f}  emit {sm[1]:.3f})   batched {b:8.3f} ms ({b / n:7.3f}; passes count {bm[0]:.3f}  emit {bm[1]:.3f})   "
                  f"batched / host {b / h:5.2f}   batched / single {b / s:5.2f}", flush=True)
    # the façade: the nine-instance file, stores built at preload and at the first render, switch off / on
    font, records = B.instance_files()["one_axis"]
    rows = {(what, on): [] for what in ("preload", "first render") for on in (False, True)}
    for run in range(args.runs + 1):
        for what in ("preload", "first render"):
            for on in (False, True):
                mgr = vg.FontManager(True)
                mgr.set_resident_commands(2)
                mgr.set_charstrings_on_device(2)
                mgr.set_charstrings_batched(on)
                mgr.add_font_named_instances(font)
                r = vg.Renderer.new_precise(0)
                w = vg.DummyWriter()
                t0 = time.perf_counter()
                if what == "preload":
                    r.preload_fonts(mgr)
                    decoded = mgr.charstring_preload_stats()["fonts_decoded"]
                else:
                    mgr.render_glyphs(w, r)
                    decoded = mgr.charstring_stats()["fonts_decoded"]
                t1 = time.perf_counter()
                assert decoded == len(records)
                if run:
                    rows[(what, on)].append(t1 - t0)
    for what in ("preload", "first render"):
        off, on = med(rows[(what, False)]), med(rows[(what, True)])
        print(f"façade, {len(records)} instances, {what:12s}  switch off {off:8.3f} ms   on {on:8.3f} ms   on / off {on / off:5.2f}", flush=True)


if __name__ == "__main__":
    main()
