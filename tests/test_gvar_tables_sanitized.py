"""The `gvar` reader under AddressSanitizer and UBSan (CPU): tests/native/gvar_tables_check.cpp, a stand-alone program, places a
glyf face at four positions and draws every glyph id both ways, for every hand-written and truncated table of
tests/gvar_instances_kit.py, for the variable Fira fixtures and for damaged copies of their gvar, glyf and fvar tables.  Nothing
sanitised is loaded into Python, and nothing of this runs on a GPU."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
from test_variation_tables_sanitized import _table_span  # noqa: E402


def _damaged(font, rng, i):
    """a copy with its gvar (mostly), glyf or fvar damaged the i-th way (the directory's checksum is not looked at by the reader)"""
    b = bytearray(font)
    rec, (off, ln) = _table_span(font, (b"gvar", b"gvar", b"gvar", b"glyf", b"fvar")[i % 5])
    way = (i // 5) % 3
    if way == 0:                                          # truncated: the directory says the table is shorter
        struct.pack_into(">I", b, rec + 12, int(rng.integers(0, ln)))
    elif way == 1:                                        # random bytes inside
        for _ in range(int(rng.integers(1, 10))):
            b[off + int(rng.integers(0, ln))] = int(rng.integers(0, 256))
    else:                                                 # an offset, count or flag field at its extremes
        at = off + 2 * int(rng.integers(0, min(ln // 2, 60)))
        struct.pack_into(">H", b, at, int(rng.choice([0, 1, 0x7FFF, 0x8000, 0xFFFF])))
    return bytes(b)


def test_gvar_reader_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "gvar_tables_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "gvar_tables_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    edge, unreadable = G.edge_faces(), G.unreadable_gvars()
    fonts = {name: f for name, (f, _) in edge.items()}
    fonts.update({"unreadable_" + name: f for name, f in unreadable.items()})
    fonts["shear"] = G.variable_glyf_fira("shear")
    fonts["two_axes"] = G.variable_glyf_fira("two_axes")
    rng = np.random.default_rng(23)
    for b, base in enumerate(("two_axes", "inference", "composites", "point_numbers", "truncated", "scalars")):
        for i in range(30):
            fonts[f"mutant_{b}_{i}"] = _damaged(fonts[base], rng, i)
    paths = []
    for name, data in fonts.items():
        p = tmp_path / (name + ".ttf")
        p.write_bytes(data)
        paths.append(str(p))
    run = subprocess.run([str(exe), "4", "16384", "8192", "-8192", "5000", *paths], capture_output=True, text=True, timeout=240)
    lines = dict(line.split(": ", 1) for line in run.stdout.splitlines())
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert len(lines) == len(paths)
    for name in edge:
        assert lines[str(tmp_path / (name + ".ttf"))].startswith("placed"), name
    for name in unreadable:
        assert lines[str(tmp_path / ("unreadable_" + name + ".ttf"))].startswith("refused"), name
    assert lines[str(tmp_path / "shear.ttf")].startswith("placed 1 315 ") and lines[str(tmp_path / "two_axes.ttf")].startswith("placed 2 315 ")
    # the malformed glyph ids of the truncated face return false at every position (its first and last glyph id do not)
    n_cuts = int(lines[str(tmp_path / "truncated.ttf")].split()[2])
    assert int(lines[str(tmp_path / "truncated.ttf")].split()[3]) == 4 * (n_cuts - 2 + 2)        # (+ 2: the ids past numGlyphs)
    print(sum(v.startswith("placed") for v in lines.values()), "placed,", sum(v.startswith("refused") for v in lines.values()),
          "refused,", sum(v == "no fvar" for v in lines.values()), "without fvar")
