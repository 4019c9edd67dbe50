"""Device span of one submission (HIP events around upload ... last kernel, VGSDF_TRACE) and end-to-end time of the same run,
config 2 (Noto Sans Regular) or another workload, over N warm runs: median / min of both.  Development aid.
    python tools/device_span.py [noto_regular|noto_all|fira|many|noto_cff] [runs] [resident] [commands|commands1]
`resident`: with resident fonts on (the first run, which builds the tables and uploads the fonts, is printed separately).
`commands`: every group by name against command stores (vg_manager_set_resident_commands 2); `commands1`: mode 1, the groups
without a glyf form only.  noto_cff: Noto Sans Regular re-encoded as CFF with fontTools (as tools/cff_time.py does)."""
import os
import re
import subprocess
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
if os.environ.get("_VG_SPAN_CHILD") != "1":
    env = dict(os.environ, VGSDF_TRACE="1", _VG_SPAN_CHILD="1")
    cp = subprocess.run([sys.executable, __file__] + sys.argv[1:], env=env, capture_output=True, text=True)
    spans = [float(m) for m in re.findall(r"device span of the submission.*?: ([0-9.]+) us", cp.stderr)]
    warm = spans[len(spans) // 3:]
    warm.sort()
    sys.stdout.write(cp.stdout)
    if warm:
        print(f"device span over {len(warm)} warm submissions: min {warm[0]:.1f} us, median {warm[len(warm) // 2]:.1f} us, p90 {warm[int(len(warm) * 0.9)]:.1f} us")
    else:
        print(cp.stderr[-2000:])
    sys.exit(cp.returncode)
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from conftest import FIRA, NOTO, load_product, noto_files  # noqa: E402
vg = load_product()
which = sys.argv[1] if len(sys.argv) > 1 else "noto_regular"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 60
resident = "resident" in sys.argv[3:]
m = vg.FontManager(True)
m.set_resident_fonts(resident)
commands = 2 if "commands" in sys.argv[3:] else 1 if "commands1" in sys.argv[3:] else 0
m.set_resident_commands(commands)
if which == "noto_cff":
    from fontTools.pens.t2CharStringPen import T2CharStringPen
    from fontTools.ttLib import TTFont
    import test_cff_outlines as T
    src = TTFont(NOTO); gs = src.getGlyphSet(); order = src.getGlyphOrder(); cs = {}
    for g in order:
        pen = T2CharStringPen(gs[g].width, gs); gs[g].draw(pen); cs[g] = pen.getCharString()
    m.add_font_data("Some Font", T._build(order, dict(src.getBestCmap()), cs, {g: gs[g].width for g in order}, src["head"].unitsPerEm))
elif which == "many":
    for i, p in enumerate([FIRA] + list(noto_files())):
        m.add_font_with_name(f"Font {i:02d}", [p])
else:
    m.add_font_with_name("Some Font", {"noto_regular": [NOTO], "fira": [FIRA], "noto_all": noto_files()}[which])
r = vg.Renderer.new_precise(0)
ts = []
for i in range(runs):
    t0 = time.perf_counter()
    m.render_glyphs(None, r)
    ts.append(time.perf_counter() - t0)
tm = m.timings()
w = sorted(ts[runs // 3:])
if commands:
    print(f"command stores (mode {commands}): first run {ts[0] * 1e6:.0f} us (tables + store upload), last run's stats {m.command_stats()}")
if resident:
    print(f"resident fonts: first run {ts[0] * 1e6:.0f} us (tables + font upload), last run's stats {m.resident_stats()}")
print(f"{which}: {tm['glyphs']} glyphs, end to end min {w[0] * 1e6:.0f} us ({tm['glyphs'] / w[0] / 1e6:.2f} M glyphs/s), median {w[len(w) // 2] * 1e6:.0f} us; "
      f"phases of the last run: " + " ".join(f"{k[:-2]}={v * 1e6:.0f}" for k, v in tm.items() if k.endswith("_s")))
