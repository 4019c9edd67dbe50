"""Rule G7's streaming walk under AddressSanitizer and UBSan (CPU): tests/native/phantom_advances_check.cpp, a stand-alone program,
places a glyf face with advances from gvar's phantom points at four positions and asks every glyph id's delta and advance, for
every hand-written face of tests/phantom_advances_kit.py, every truncation of their gvar tables and damaged copies of six of them.
For every glyph id visited the program also holds GvarTable::phantom_sums against GvarTable::accumulate (same glyph id, position
and point count, no contours): malformed to one exactly where malformed to the other, and l / r the 32 bits of the outline's x sums
of points n and n + 1 (G7 pinned against G1 to G5 directly).
Nothing sanitised is loaded into Python, and nothing of this runs on a GPU."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytest.importorskip("fontTools")

import phantom_advances_kit as P  # noqa: E402
from test_gvar_tables_sanitized import _damaged  # noqa: E402
from test_variation_tables_sanitized import _table_span  # noqa: E402


def test_phantom_advances_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "phantom_advances_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "phantom_advances_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    hand = {name: f for name, (f, _) in P.faces().items()}
    hand["truncated"] = P.truncated_face()
    hand["over_budget"] = P.over_budget_face()
    fonts = dict(hand)
    n_cuts = 0
    for name, font in hand.items():                        # every truncation of the gvar table: the directory says it is shorter
        rec, (_, ln) = _table_span(font, b"gvar")
        for k in range(ln):
            b = bytearray(font)
            struct.pack_into(">I", b, rec + 12, k)
            fonts[f"cut_{name}_{k}"] = bytes(b)
            n_cuts += 1
    fonts["fira"] = P.without_hvar("shear")
    rng = np.random.default_rng(29)
    for b, base in enumerate(("point_lists", "delta_runs", "scalars", "composites", "malformed", "truncated")):
        for i in range(30):
            fonts[f"mutant_{b}_{i}"] = _damaged(hand[base], rng, i)
    paths = []
    for name, data in fonts.items():
        p = tmp_path / (name + ".ttf")
        p.write_bytes(data)
        paths.append(str(p))
    run = subprocess.run([str(exe), "4", "16384", "8192", "-8192", "5000", *paths], capture_output=True, text=True, timeout=240)
    lines = dict(line.split(": ", 1) for line in run.stdout.splitlines())
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert len(lines) == len(paths) and n_cuts > 2000
    for name in hand:
        assert lines[str(tmp_path / (name + ".ttf"))].startswith("placed 1 "), name
    # the fixture: 315 glyph ids with data at each of the four positions, none malformed; every advance moved at 16384 and at 8192
    # (-8192 lies below the axis' default: every tuple's scalar is 0 there)
    fira = lines[str(tmp_path / "fira.ttf")].split()
    assert fira[:5] == ["placed", "1", "315", str(4 * 315), "0"] and 2 * 315 <= int(fira[5]) <= 3 * 315
    # the truncated face: every cut but none and all of the data is malformed at each position
    cuts = lines[str(tmp_path / "truncated.ttf")].split()
    assert int(cuts[4]) == 4 * (int(cuts[2]) - 2)
    print(sum(v.startswith("placed") for v in lines.values()), "placed,", sum(v.startswith("refused") for v in lines.values()),
          "refused,", sum(v == "no fvar" for v in lines.values()), "without fvar")
