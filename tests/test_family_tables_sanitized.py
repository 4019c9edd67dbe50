"""Face::family_tables() under AddressSanitizer and UBSan (CPU): tests/native/family_tables_check.cpp, a stand-alone program,
builds the description of cmap and hmtx for the fixture fonts, for the edge tables of tests/cmap_edge_tables.py spliced into a
fixture font, and for seeded damaged copies — truncated tables, subtable offsets at and past the end of the table, segCountX2 and
group counts that overrun.  Nothing sanitised is loaded into Python, and nothing of this runs on a GPU."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import FIRA, ROOT, noto_files

pytest.importorskip("fontTools")

import cmap_edge_tables as E  # noqa: E402
from test_family_tables_desc_host import splice  # noqa: E402


def _damaged(face, rng, i):
    """a copy of the face with its cmap damaged the i-th way"""
    f = dict(face)
    cmap = bytearray(f["cmap"])
    n = E.u16(cmap, 2)
    subs = [E.u32(cmap, 8 + 8 * k) for k in range(n)]
    way = i % 6
    if way == 0 and len(cmap) > 8:                                       # truncated
        cmap = cmap[:int(rng.integers(4, len(cmap)))]
    elif way == 1 and n:                                                 # a subtable offset at / past the end
        struct.pack_into(">I", cmap, 8 + 8 * int(rng.integers(0, n)), len(cmap) + int(rng.integers(0, 3)) * int(rng.integers(0, 1 << 20)))
    elif way == 2 and n:                                                 # segCountX2 / the group count overruns
        o = subs[int(rng.integers(0, n))]
        if o + 16 <= len(cmap):
            if E.u16(cmap, o) == 4:
                struct.pack_into(">H", cmap, o + 6, int(rng.choice([0, 1, 0xFFFE, 0xFFFF, 2 * len(cmap)])) & 0xFFFF)
            else:
                struct.pack_into(">I", cmap, o + 12, int(rng.choice([0xFFFFFFFF, len(cmap), len(cmap) // 12 + 1, 0x15555556])))
    elif way == 3 and n:                                                 # the two bytes behind the last subtable's start
        o = subs[-1]
        cmap = cmap[:min(o + int(rng.integers(0, 20)), len(cmap))]
    elif way == 4:                                                       # random bytes
        for _ in range(int(rng.integers(1, 12))):
            cmap[int(rng.integers(0, len(cmap)))] = int(rng.integers(0, 256))
    else:                                                                # hmtx truncated, counts that disagree
        f["hmtx"] = f["hmtx"][:int(rng.integers(0, len(f["hmtx"]) + 1))]
        f["num_hmetrics"] = int(rng.choice([0, 1, f["num_hmetrics"], 0xFFFF]))
        f["num_glyphs"] = int(rng.choice([0, 1, f["num_glyphs"], 0xFFFF]))
    f["cmap"] = bytes(cmap)
    return f


def test_family_tables_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    host = ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "host"
    exe = tmp_path / "family_tables_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", str(host), str(ROOT / "tests" / "native" / "family_tables_check.cpp"),
           str(host / "ttf_face.cpp"), str(host / "cff.cpp"), "-o", str(exe)]
    # the sanitizer runtimes are probed for with an empty program first: a failure of the project's own build is a failure
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("sanitizer runtimes not available: " + probed.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    regular = {f"{name}_{k}": f for name, faces in E.regular_cases().items() for k, f in enumerate(faces)}
    irregular = E.irregular_cases()
    fonts = {name: splice(f) for name, f in {**regular, **irregular}.items()}
    rng = np.random.default_rng(5)
    bases = [regular["format4_range_offsets_0"], regular["format12_0"], regular["skipped_records_0"], regular["two_subtables_0"],
             regular["format6_0"], regular["format10_0"], regular["format4_64_segments_0"]]
    for b, base in enumerate(bases):
        for i in range(18):
            fonts[f"mutant_{b}_{i}"] = splice(_damaged(base, rng, i))
    paths = []
    for name, data in fonts.items():
        p = tmp_path / (name + ".ttf")
        p.write_bytes(data)
        paths.append(str(p))
    fixtures = [str(FIRA)] + [str(p) for p in noto_files()]
    paths += fixtures
    run = subprocess.run([str(exe), *paths], capture_output=True, text=True, timeout=240)
    lines = dict(line.rsplit(": ", 1) for line in run.stdout.splitlines())
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert len(lines) == len(paths)
    for name in regular:
        assert lines[str(tmp_path / (name + ".ttf"))].startswith("described"), name
    for name in irregular:
        assert lines[str(tmp_path / (name + ".ttf"))].startswith("refused"), name
    for p in fixtures:
        assert lines[p].startswith("described"), p
    print(sum(v.startswith("described") for v in lines.values()), "described,", sum(v.startswith("refused") for v in lines.values()),
          "refused,", sum(v == "not a font" for v in lines.values()), "not fonts")
