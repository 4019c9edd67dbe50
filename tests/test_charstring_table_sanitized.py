"""Face::charstring_table() under AddressSanitizer and UBSan (CPU): tests/native/charstring_table_check.cpp, a stand-alone
program, builds the description for synthesised and for damaged `CFF ` fonts written to a temporary directory.  Nothing
sanitised is loaded into Python, and nothing of this runs on a GPU."""
import shutil
import subprocess

import numpy as np
import pytest

from conftest import FIRA, ROOT

pytest.importorskip("fontTools")

import charstring_edge_programs as K  # noqa: E402
from test_cff_outlines import fira_cff, ops_cff  # noqa: E402,F401  (fixtures)
from test_resident_commands_host import _cff2, _damage  # noqa: E402


def test_charstring_table_under_asan_and_ubsan(tmp_path, fira_cff, ops_cff):  # noqa: F811
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "charstring_table_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "charstring_table_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    # the sanitizer runtimes are probed for with an empty program first: a failure of the project's own build is a failure
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    fonts = {"fira_cff": fira_cff, "ops_cff": ops_cff, "cff2": _cff2(), "shared": K.shared_face().font(), "cid": K.cid_face().font(),
             "small_os1": K.sized_face(3).font(off_size=1), "small_os4": K.sized_face(3).font(off_size=4),
             "global_33900": K.bias_faces()[3].font(), "empty_glyphs": K.sized_face(129, empty=set(range(0, 129, 2))).font()}
    rng = np.random.default_rng(3)
    for base in ("fira_cff", "cid", "shared"):
        for i in range(1, 25):
            fonts[f"{base}_mutant_{i}"] = _damage(fonts[base], rng, i)
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
    for name in ("fira_cff", "ops_cff", "shared", "cid", "small_os1", "small_os4", "global_33900", "empty_glyphs"):
        assert lines[str(tmp_path / (name + ".otf"))].startswith("described"), name
    assert lines[str(tmp_path / "cff2.otf")] == "no description" and lines[str(FIRA)] == "no description"
    print(sum(v.startswith("described") for v in lines.values()), "described,", sum(v == "no description" for v in lines.values()),
          "without, ", sum(v == "not a font" for v in lines.values()), "not fonts")
