"""The readers behind vg_manager_add_font_named_instances under AddressSanitizer and UBSan (CPU):
tests/native/named_instances_check.cpp, a stand-alone program, reads the fvar instance records (with and without
postScriptNameID) and the name table of the files of tests/named_instances_kit.py, whole and at EVERY truncation of the two
tables, each cut made the end of the program's allocation.  The names it prints for the whole files are the restatement's.
Nothing sanitised is loaded into Python, and nothing of this runs on a GPU."""
import shutil
import subprocess

import pytest

from conftest import FIRA, ROOT

pytest.importorskip("fontTools")

import named_instances_kit as N  # noqa: E402
from test_variation_tables_sanitized import _table_span  # noqa: E402


def test_instance_and_name_readers_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "named_instances_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "named_instances_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    fonts = {name: font for name, (font, _) in N.files().items()}
    fonts["bare"] = N.no_instances(fonts["edge"])
    paths = {}
    for name, data in fonts.items():
        paths[name] = tmp_path / (name + ".ttf")
        paths[name].write_bytes(data)
    run = subprocess.run([str(exe), *map(str, paths.values()), str(FIRA)], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    lines = dict(line.split(": ", 1) for line in run.stdout.splitlines())
    assert len(lines) == len(paths) + 1 and lines[str(FIRA)] == "no fvar"
    for name, font in fonts.items():
        head, *strings = lines[str(paths[name])].split("|")
        state, n_axes, n_instances, cuts = head.split()
        family, names = N.ps_names(font)
        assert state == "ok" and int(n_axes) == (2 if name.startswith("two_axes") else 1), name
        assert int(n_instances) == len(names) and strings == [family] + names, name
        # every length of fvar and of name, 0 and the whole table included
        assert int(cuts) == sum(_table_span(font, tag)[1][1] + 1 for tag in (b"fvar", b"name")), name
