"""Host halves of the resident-font form (CPU): what vgsdf_font_create and vgsdf_outlines_submit_resident are handed.

`resident_font_desc` describes one file of a font id — the leaves (simple glyphs + accumulated transforms) of EVERY glyph id,
each simple glyph's arrays stored once — and `record_resident` names every glyph of the font id by (file, glyph id).  Expanding
the names with the descriptions, as the upload kernel does on the device (part = leaf, cmd_at += cmd_off[g], bytes addressed in
the font's store), must give part for part what `record_glyf_parts` records for the same font: same slots, same transforms,
byte-equal arrays.  The glyf form is itself pinned to the host's reader by tests/test_glyf_parts_host.py.
"""
import subprocess

import numpy as np
import pytest

from conftest import FIRA, NOTO, NOTO_DIR, ROOT, noto_files

FONT_SETS = {
    "fira": [FIRA],
    "noto_regular": [NOTO],
    "noto_all": None,   # the 20 files, canonical order
    "arabic": [NOTO_DIR / "Noto Sans Arabic - Regular.ttf"],     # these two hold the components with a 2 x 2 transform
    "myanmar": [NOTO_DIR / "Noto Sans Myanmar - Regular.ttf"],
}


def expand(rec, descs):
    """numpy model of the device's expansion -> (cmd_off, part_off, parts with cmd_at in the batch, font of every part)"""
    n = len(rec["glyph_id"])
    counts = np.zeros(n, dtype=np.int64)
    slots = np.zeros(n, dtype=np.int64)
    first = np.zeros(n, dtype=np.int64)
    for k, d in enumerate(descs):
        sel = rec["font_of"] == k
        gid = rec["glyph_id"][sel].astype(np.int64)
        lo, hi = d["leaf_off"][gid].astype(np.int64), d["leaf_off"][gid + 1].astype(np.int64)
        counts[sel], first[sel] = hi - lo, lo
        ends = np.concatenate([[0], np.cumsum(d["leaves"]["cmd_cap"].astype(np.int64))])
        slots[sel] = ends[hi] - ends[lo]
    part_off = np.concatenate([[0], np.cumsum(counts)])
    cmd_off = np.concatenate([[0], np.cumsum(slots)])
    glyph_of_part = np.repeat(np.arange(n), counts)
    k_in_glyph = np.arange(int(part_off[-1])) - part_off[glyph_of_part]
    font_of_part = rec["font_of"][glyph_of_part]
    parts = np.zeros(int(part_off[-1]), dtype=descs[0]["leaves"].dtype)
    for k, d in enumerate(descs):
        sel = font_of_part == k
        parts[sel] = d["leaves"][first[glyph_of_part[sel]] + k_in_glyph[sel]]
    parts["cmd_at"] = (parts["cmd_at"].astype(np.int64) + cmd_off[glyph_of_part]).astype(np.uint32)
    return cmd_off.astype(np.uint32), part_off, parts, font_of_part


def assert_expands_to_the_glyf_form(mgr, fid):
    g = mgr.record_glyf_parts(fid)
    r = mgr.record_resident(fid)
    descs = [mgr.resident_font_desc(fid, k) for k in range(r["n_files"])]
    for key in ("ids", "advances", "scale", "shift_x"):
        assert np.array_equal(g[key], r[key]), key
    for d in descs:
        lv = d["leaves"]
        assert d["leaf_off"][0] == 0 and d["leaf_off"][-1] == len(lv) and (np.diff(d["leaf_off"].astype(np.int64)) >= 0).all()
        assert len(d["bytes"]) % 4 == 0 and (lv["byte_off"] % 4 == 0).all() and (lv["n_contours"] > 0).all() and (lv["plain"] <= 1).all()
        assert (lv["byte_off"].astype(np.int64) + lv["byte_len"] <= len(d["bytes"])).all()
        # the leaves of a glyph tile its slots from 0
        starts = np.zeros(len(lv), dtype=bool)
        starts[d["leaf_off"][:-1][np.diff(d["leaf_off"].astype(np.int64)) > 0]] = True
        ends = lv["cmd_at"].astype(np.int64) + lv["cmd_cap"]
        assert (lv["cmd_at"][starts] == 0).all() and (lv["cmd_at"][1:][~starts[1:]] == ends[:-1][~starts[1:]]).all()
    cmd_off, part_off, parts, font_of_part = expand(r, descs)
    want = g["parts"]
    assert np.array_equal(cmd_off, g["cmd_off"]) and len(parts) == len(want)
    for field in ("cmd_at", "cmd_cap", "n_contours", "plain", "byte_len"):
        assert np.array_equal(parts[field], want[field]), field
    for field in "abcdef":
        assert parts[field].tobytes() == want[field].tobytes(), field
    # byte-equal arrays behind byte_off
    for i in range(len(parts)):
        a, b, ln = int(parts["byte_off"][i]), int(want["byte_off"][i]), int(want["byte_len"][i])
        assert descs[int(font_of_part[i])]["bytes"][a:a + ln].tobytes() == g["bytes"][b:b + ln].tobytes(), i
    return g, r, descs


@pytest.mark.parametrize("which", list(FONT_SETS))
def test_names_expand_to_the_parts_of_the_glyf_form(vg, which):
    paths = FONT_SETS[which] or noto_files()
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Font", paths)
    g, r, descs = assert_expands_to_the_glyf_form(mgr, fid)
    assert r["n_files"] == len(paths) and len(r["ids"]) > 200
    if which == "fira":
        # the store holds each simple glyph once: below what the parts of the glyf form copy per run
        assert len(descs[0]["bytes"]) == 90328 and len(g["bytes"]) == 145668
    if which == "noto_all":
        assert len(np.unique(r["font_of"])) == 20
    if which in ("arabic", "myanmar"):   # components with a 2 x 2 transform are among the leaves
        lv = descs[0]["leaves"]
        assert int(((lv["b"] != 0) | (lv["c"] != 0) | (lv["a"] != 1) | (lv["d"] != 1)).sum()) >= 1


def _glyf_table_length(path):
    font = path.read_bytes()
    for i in range(int.from_bytes(font[4:6], "big")):
        rec = 12 + 16 * i
        if font[rec:rec + 4] == b"glyf":
            return int.from_bytes(font[rec + 12:rec + 16], "big")
    raise AssertionError("no glyf table")


@pytest.mark.parametrize("path", [FIRA] + noto_files(), ids=lambda p: p.stem.replace(" ", ""))
def test_the_store_holds_each_simple_glyph_once(vg, path):
    """n_bytes of a description is at most the length of the face's `glyf` table (an entry minus its header and instructions,
    padded to 4, no entry twice): 0.41 (Fira) to 0.94 (Sinhala) of it for the fixture fonts"""
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Font", [path])
    d = mgr.resident_font_desc(fid, 0)
    assert 0 < len(d["bytes"]) <= _glyf_table_length(path)
    # no two leaves of different entries overlap, and equal offsets mean equal lengths (one entry, stored once)
    lv = d["leaves"]
    first = {}
    for off, ln in zip(lv["byte_off"].tolist(), lv["byte_len"].tolist()):
        assert first.setdefault(off, ln) == ln
    offs = np.array(sorted(first), dtype=np.int64)
    lens = np.array([first[o] for o in offs], dtype=np.int64)
    assert (offs[:-1] + lens[:-1] <= offs[1:]).all() and int(((lens + 3) // 4 * 4).sum()) == len(d["bytes"])


def test_fan_out_fonts(vg):
    pytest.importorskip("fontTools")
    from test_composite_fanout import fan_out_font
    # a modest fan-out: 13 leaves over 4 glyph ids, the one simple glyph they all name stored once
    small = vg.FontManager(False)
    fid = small.add_font_data("Fan Small", fan_out_font(points=200, fan=3))
    _, r, descs = assert_expands_to_the_glyf_form(small, fid)
    d = descs[0]
    assert list(np.diff(d["leaf_off"])) == [1, 1, 3, 9] and len(np.unique(d["leaves"]["byte_off"][1:])) == 1
    assert len(d["bytes"]) < 2 * (2 + 200 * 5 + 8)
    # past the bounds (90 000 leaves of 1502 slots under one glyph id): no resident form, and no gigabytes on the way
    import resource
    big = vg.FontManager(False)
    fid = big.add_font_data("Fan Out", fan_out_font())
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    with pytest.raises(RuntimeError, match="fan-out"):
        big.resident_font_desc(fid, 0)
    with pytest.raises(RuntimeError, match="fan-out"):
        big.record_resident(fid)
    assert (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) / 1024 < 400


def test_faces_without_glyf_outlines_have_no_resident_form(vg):
    pytest.importorskip("fontTools")
    from test_cff2_outlines import _GLOBAL, _LOCAL, _NAMES, _PROGS, _build2
    cff2 = _build2(_NAMES, _PROGS, local_subrs=_LOCAL, global_subrs=_GLOBAL, extra_vardata=[(3, 0)])
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("CFF2", cff2)
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.resident_font_desc(fid, 0)
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.record_resident(fid)
    with pytest.raises(RuntimeError):
        mgr.resident_font_desc("no_such_font", 0)


_C_PROGRAM = r"""
/* a plain C caller builds a font description and walks it (no device needed) */
#include <stdio.h>
#include "vgsdf.h"
#include "vgfont.h"
int main(int argc, char **argv)
{
	vg_manager *m = vg_manager_new(0);
	const char *files[1];
	vgsdf_font_desc d;
	vg_resident_batch *rb;
	vg_resident_view v;
	uint32_t g, i, n_parts = 0;
	if (argc < 2 || !m)
		return 2;
	files[0] = argv[1];
	if (vg_manager_add_font_with_name(m, "Fira Sans Regular", files, 1) < 0 || vg_manager_resident_font_desc(m, "fira_sans_regular", 0, &d) != 0) {
		fprintf(stderr, "desc: %s\n", vg_last_error());
		return 1;
	}
	for (g = 0; g < d.n_glyph_ids; g++) {
		uint32_t slots = 0;
		for (i = d.leaf_off[g]; i < d.leaf_off[g + 1]; i++) {
			const vgsdf_glyf_part *lf = &d.leaves[i];
			if (lf->cmd_at != slots || lf->byte_off % 4 || lf->byte_off + lf->byte_len > d.n_bytes || lf->n_contours == 0)
				return 3;
			slots += lf->cmd_cap;
		}
	}
	if (d.leaf_off[0] != 0 || d.leaf_off[d.n_glyph_ids] != d.n_leaves || d.n_bytes % 4)
		return 4;
	rb = vg_manager_record_resident(m, "fira_sans_regular");
	if (!rb || vg_resident_batch_view(rb, &v) != 0 || v.n_files != 1 || v.n_glyphs < 1000 || v.ids[0] != 13)
		return 5;
	for (g = 0; g < v.n_glyphs; g++) {
		if (v.font_of[g] != 0 || v.glyph_id[g] >= d.n_glyph_ids)
			return 6;
		n_parts += d.leaf_off[v.glyph_id[g] + 1] - d.leaf_off[v.glyph_id[g]];
	}
	printf("leaves %u of %u glyph ids, %u bytes; %u glyphs name %u parts\n", (unsigned)d.n_leaves, (unsigned)d.n_glyph_ids,
	       (unsigned)d.n_bytes, (unsigned)v.n_glyphs, (unsigned)n_parts);
	vg_resident_batch_free(rb);
	vg_manager_free(m);
	return 0;
}
"""


def test_the_new_declarations_are_plain_c(vg, tmp_path):
    """include/*.h still compile as C99 -pedantic -Werror; a plain C program builds a description and walks it"""
    src = tmp_path / "resident.c"
    src.write_text(_C_PROGRAM)
    exe = tmp_path / "resident"
    lib = vg.lib_path()
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    f"-L{lib.parent}", f"-l:{lib.name}", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe), str(FIRA)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    # Fira: 1686 glyphs name the 2538 parts the glyf form records, and the store is the 90 328 bytes of its simple glyphs
    assert "1686 glyphs name 2538 parts" in p.stdout and "90328 bytes" in p.stdout


def test_a_font_past_the_bounds_renders_to_the_same_files_with_the_switch_on(vg):
    """no resident form: the switch changes nothing about what is written (dummy renderer: runs without a GPU)"""
    pytest.importorskip("fontTools")
    from test_composite_fanout import fan_out_font
    font = fan_out_font(points=760)   # (762 slots x 90 000 leaves under one glyph id: past 2^26)
    files = {}
    for on in (False, True):
        mgr = vg.FontManager(True)
        mgr.set_resident_fonts(on)
        fid = mgr.add_font_data("Fan Out", font)
        if on:
            with pytest.raises(RuntimeError, match="fan-out"):
                mgr.resident_font_desc(fid, 0)
        w = vg.DummyWriter()
        mgr.render_glyphs(w, vg.Renderer.new_dummy())
        files[on] = w.files
        assert mgr.resident_stats() == {"groups": 0, "fonts_uploaded": 0, "font_bytes": 0, "block_bytes": 0}
    assert files[True] == files[False] and len(files[True]) >= 256
