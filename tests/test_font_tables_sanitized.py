"""Face::font_tables() under AddressSanitizer and UBSan (CPU): tests/native/font_tables_check.cpp, a stand-alone program, builds
the description of loca and glyf — and the host's table from the same bytes — for the fixture fonts, for the edge fonts of
tests/composite_edge_trees.py and for the seeded damaged copies of tests/test_font_tables_desc_host.py.  Nothing sanitised is
loaded into Python, and nothing of this runs on a GPU."""
import shutil
import subprocess

import pytest

from conftest import FIRA, ROOT, noto_files

pytest.importorskip("fontTools")

import composite_edge_trees as T  # noqa: E402
from test_font_tables_desc_host import mutants  # noqa: E402


def test_font_tables_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "font_tables_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "font_tables_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    # the sanitizer runtimes are probed for with an empty program first: a failure of the project's own build is a failure
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    tables = {name: T.case_tables(name) for name in T.LONG_CASES}
    tables.update({name: t for name, t in T.LOCA_FONTS.items() if name not in ("no_loca", "no_glyf")})
    tables.update({"budget_at": T.budget_font(0), "budget_past": T.budget_font(1), "slots_at": T.slots_font(1023), "slots_past": T.slots_font(1024),
                   "leaves_at": T.leaves_font(0), "leaves_past": T.leaves_font(1),
                   "count_129_deep_last": T.count_font(129, 128), "side_by_side": T.forest_of(T.LONG_CASES).tables()})
    tables.update(dict(mutants()))
    paths = []
    for name, t in tables.items():
        p = tmp_path / (name + ".ttf")
        p.write_bytes(T.font_of(t))
        paths.append(str(p))
    fixtures = [str(FIRA)] + [str(p) for p in noto_files()]
    run = subprocess.run([str(exe), *paths, *fixtures], capture_output=True, text=True, timeout=600)
    lines = dict(line.rsplit(": ", 1) for line in run.stdout.splitlines())
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert len(lines) == len(paths) + len(fixtures)
    for name, t in tables.items():
        words = lines[str(tmp_path / (name + ".ttf"))].split()
        mine = T.restate(t)
        assert words[0] == "described" and (int(words[1]), int(words[2])) == (t.num_glyphs, t.loca_entries), name
        assert words[4] == ("refused" if mine == T.REFUSED_BOUNDS else words[4]), name
        if not isinstance(mine, str):
            assert int(words[4]) == len(mine["leaves"]), name
    for p in fixtures:
        assert lines[p].startswith("described") and not lines[p].endswith("refused"), p
    print(sum(v.endswith("refused") for v in lines.values()), "of", len(lines), "tables refused")
