"""Face::charstring2_table() under AddressSanitizer and UBSan (CPU): tests/native/charstring2_table_check.cpp, a stand-alone
program, builds the description of the variable Fira face (CFF2, merged by fontTools.varLib), of the kit's hand-written tables and
of copies with seeded byte damage inside the `CFF2` table, all written to a temporary directory.  Nothing sanitised is loaded
into Python, and nothing of this runs on a GPU."""
import shutil
import subprocess

import numpy as np
import pytest

from conftest import FIRA, ROOT

pytest.importorskip("fontTools")

import charstring2_edge_programs as K2  # noqa: E402
from fira_cff_kit import fira_as_cff  # noqa: E402
from test_cff2_outlines import _variable_fira  # noqa: E402


def _damage_cff2(font, rng, i):
    """byte damage inside the CFF2 table: header / Top DICT / INDEX offsets at its start, charstrings and the store further in"""
    at = font.index(b"CFF2")
    off, ln = int.from_bytes(font[at + 8:at + 12], "big"), int.from_bytes(font[at + 12:at + 16], "big")
    b = bytearray(font)
    hi = (64, 600, ln)[i % 3]
    for pos in rng.integers(0, min(hi, ln), int(rng.integers(1, 16))):
        b[off + int(pos)] = int(rng.integers(0, 256))
    return bytes(b)


def test_charstring2_table_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "charstring2_table_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "charstring2_table_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    # the sanitizer runtimes are probed for with an empty program first: a failure of the project's own build is a failure
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    fonts = {"fira_cff2": _variable_fira(), "shared2": K2.shared_face().font(), "no_sets": K2.no_sets_face().font(),
             "set0_unusable": K2.set0_unusable_face().font(), "sized2": K2.sized_face(65).font(), "fira_cff": fira_as_cff(40)}
    rng = np.random.default_rng(3)
    for base in ("fira_cff2", "shared2"):
        for i in range(1, 61):
            fonts[f"{base}_mutant_{i}"] = _damage_cff2(fonts[base], rng, i)
    paths = []
    for name, data in fonts.items():
        p = tmp_path / (name + ".otf")
        p.write_bytes(data)
        paths.append(str(p))
    paths.append(str(FIRA))
    run = subprocess.run([str(exe), *paths], capture_output=True, text=True, timeout=240)
    lines = dict(line.rsplit(": ", 1) for line in run.stdout.splitlines())
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert len(lines) == len(paths)
    for name in ("fira_cff2", "shared2", "no_sets", "set0_unusable", "sized2"):
        assert lines[str(tmp_path / (name + ".otf"))].startswith("described"), name
    assert lines[str(tmp_path / "fira_cff.otf")] == "no description" and lines[str(FIRA)] == "no description"
    n_described = sum(v.startswith("described") for k, v in lines.items() if "_mutant_" in k)
    print(n_described, "mutants described,", sum(v == "no description" for v in lines.values()), "without a description,",
          sum(v == "not a font" for v in lines.values()), "not fonts")
    assert n_described >= 10
