"""Timings of variable-font instances (vg_manager_add_font_instance), the forms alternating in one process, every run on a fresh
Renderer and a fresh FontManager (so stores, families and the host's tables are built in the timed span: the first render of an
instance is what is measured), medians of --runs:
  (1) the family table of an instance built by the host (FontManager::family_table, advances through Face::glyph_hor_advance
      and HVAR) against built by the device (vgsdf_family_create_tables_var), through the façade, and at the C ABI with the count
      and emit passes' own times from HIP events (vgsdf_family_tables_kernel_ms);
  (2) the instance's command store from the host reader's table against decoded on the device (set_charstrings_on_device 0 / 2);
  (3) --static [--root CHECKOUT --label NAME]: the first render of the same files added plainly (no position), with the package
      of CHECKOUT (default: this one), for an A/B between two checkouts — the fixtures always come from this checkout's kit, so a
      checkout from before this tool can be measured: run the two in turn, process by process (nothing on that path differs
      between them, so no difference is expected).
Inputs: the variable Fira fixtures of tests/variable_instances_kit.py, 300 glyphs, one axis at wght 650 and two axes at
(wght 650, wdth 150).
  python tools/variable_instances_ab.py [--runs 11] [--static [--root ../parent --label parent]]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def stats(v):
    return f"best {min(v) * 1e3:8.3f} ms  median {statistics.median(v) * 1e3:8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--root", default=str(HERE), help="with --static: the checkout whose package is measured")
    ap.add_argument("--label", default="head", help="with --static: what the lines call that checkout")
    args = ap.parse_args()
    root = Path(args.root).resolve() if args.static else HERE
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "tests"))
    sys.path.append(str(HERE / "tests"))                                             # (the kit, where root has none)
    from conftest import load_product
    vg = load_product()
    import variable_instances_kit as K
    inputs = [("one axis, wght 650", K.variable_fira(300), {"wght": 650}),
              ("two axes, wght 650 wdth 150", K.variable_fira(300, two_axes=True), K.EXACT_TWO_AXES)]

    def render_once(font, loc, commands=1, charstrings=0, families=False, tables=False):
        mgr = vg.FontManager(True)
        mgr.set_resident_commands(commands)
        mgr.set_charstrings_on_device(charstrings)
        mgr.set_resident_families(families)
        mgr.set_family_tables_on_device(tables)
        if loc is None:
            mgr.add_font_data("Timed", font)
        else:
            mgr.add_font_instance("Timed", font, loc)
        r = vg.Renderer.new_precise(0)
        w = vg.DummyWriter()
        t0 = time.perf_counter()
        mgr.render_glyphs(w, r)
        t = time.perf_counter() - t0
        if tables:
            assert mgr.family_table_stats() == {"built_on_device": 1, "fallbacks": 0}
        if charstrings == 2:
            assert mgr.charstring_stats()["fonts_decoded"] == 1
        r.close()
        return t

    if args.static:
        for name, font, _ in inputs:
            render_once(font, None)
            print(f"{args.label}: static first render of the file ({name.split(',')[0]}), commands 1: "
                  f"{stats([render_once(font, None) for _ in range(args.runs)])}")
        return

    ctx = vg.SdfContext(0)

    def abi_once(font, loc, device):
        mgr = vg.FontManager(False)
        fid = mgr.add_font_instance("Timed", font, loc)
        d = mgr.command_font_desc(fid)
        store = ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"])
        t0 = time.perf_counter()
        if device:
            fam = ctx.family_create_tables_var([store], [mgr.family_tables_desc(fid, 0)], [mgr.family_variation_desc(fid, 0)])
            ms = ctx.family_tables_kernel_ms()
        else:
            e = mgr.family_desc(fid)
            fam = ctx.family_create([store], e["code_point"], e["font_of"], e["glyph_id"], e["advance"], e["scale"], e["shift_x"])
            ms = (0.0, 0.0)
        t = time.perf_counter() - t0
        fam.free()
        store.free()
        return t, ms

    for name, font, loc in inputs:
        print(f"\n{name}: {args.runs} runs each, alternating, a fresh renderer and manager per run")
        forms = {"family table by the host  ": dict(families=True), "family table by the device": dict(families=True, tables=True)}
        for kw in forms.values():
            render_once(font, loc, **kw)                                             # warm: code, allocator, clocks
        t = {k: [] for k in forms}
        for _ in range(args.runs):
            for k, kw in forms.items():
                t[k].append(render_once(font, loc, **kw))
        for k in forms:
            print(f"  (1) first render, {k}: {stats(t[k])}")
        abi_once(font, loc, False), abi_once(font, loc, True)
        rows = {False: [], True: []}
        for _ in range(args.runs):
            for device in (False, True):
                rows[device].append(abi_once(font, loc, device))
        print(f"  (1) C ABI, description + vgsdf_family_create           : {stats([x[0] for x in rows[False]])}")
        print(f"  (1) C ABI, descriptions + vgsdf_family_create_tables_var: {stats([x[0] for x in rows[True]])} | count pass median "
              f"{statistics.median(x[1][0] for x in rows[True]):.3f} ms, emit pass (VAR) median {statistics.median(x[1][1] for x in rows[True]):.3f} ms")
        forms = {"charstrings by the host reader": dict(charstrings=0), "charstrings decoded on device ": dict(charstrings=2)}
        for kw in forms.values():
            render_once(font, loc, **kw)
        t = {k: [] for k in forms}
        for _ in range(args.runs):
            for k, kw in forms.items():
                t[k].append(render_once(font, loc, **kw))
        for k in forms:
            print(f"  (2) first render, {k}: {stats(t[k])}")
    ctx.close()


if __name__ == "__main__":
    main()
