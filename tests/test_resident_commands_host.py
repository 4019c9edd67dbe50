"""The host halves of command fonts (vg_manager_command_font_desc / vg_manager_record_resident_commands), no device needed:
for every face the reader can read — glyf, CFF, CFF2 — the description holds, glyph id by glyph id, exactly the callbacks a
render of the glyph records today.  Everything is compared as bits (uint32 views of the 28-byte records); no tolerance.
"""
import io
import subprocess

import numpy as np
import pytest

from conftest import FIRA, ROOT

fontTools = pytest.importorskip("fontTools")
from fontTools.pens.t2CharStringPen import T2CharStringPen  # noqa: E402
from fontTools.ttLib import TTFont  # noqa: E402

from test_cff_outlines import _build, ops_cff  # noqa: E402,F401  (ops_cff: the operator and subroutine font, a fixture)


@pytest.fixture(scope="module")
def fira_as_cff():
    """all of Fira Sans re-encoded as CFF (composites decomposed, quadratics raised to cubics by the pen)"""
    src = TTFont(FIRA)
    gs = src.getGlyphSet()
    order = src.getGlyphOrder()
    cs = {}
    for g in order:
        pen = T2CharStringPen(gs[g].width, gs)
        gs[g].draw(pen)
        cs[g] = pen.getCharString()
    return _build(order, dict(src.getBestCmap()), cs, {g: gs[g].width for g in order}, src["head"].unitsPerEm)


def _cff2():
    from test_cff2_outlines import _GLOBAL, _LOCAL, _NAMES, _PROGS, _build2
    return _build2(_NAMES, _PROGS, local_subrs=_LOCAL, global_subrs=_GLOBAL, extra_vardata=[(3, 0)])


def _n_floats(kinds):
    k = kinds.astype(np.int64)
    return np.select([k <= 1, k == 2, k == 3], [2, 4, 6], 0)


def expand(vg, d):
    """a description's commands as 28-byte records, every glyph's coordinates taken from ITS dat_off range"""
    from versatiles_glyphs_rs_amd.device import OUTLINE_CMD_DTYPE
    kinds, nf = d["kinds"], _n_floats(d["kinds"])
    run = np.concatenate([[0], np.cumsum(nf)])
    glyph_of = np.repeat(np.arange(len(d["cmd_off"]) - 1), np.diff(d["cmd_off"].astype(np.int64)))
    at = d["dat_off"].astype(np.int64)[glyph_of] + run[:-1] - run[d["cmd_off"].astype(np.int64)[glyph_of]]
    out = np.zeros(len(kinds), dtype=OUTLINE_CMD_DTYPE)
    out["kind"] = kinds
    c = np.concatenate([d["coords"], np.zeros(6, np.float32)])
    for fields, n in ((("x", "y"), 2), (("x1", "y1", "x", "y"), 4), (("x1", "y1", "x2", "y2", "x", "y"), 6)):
        sel = nf == n
        for j, f in enumerate(fields):
            out[f][sel] = c[at[sel] + j]
    return out


def assert_invariants(d, n_glyph_ids):
    cmd_off, dat_off = d["cmd_off"].astype(np.int64), d["dat_off"].astype(np.int64)
    assert len(cmd_off) == len(dat_off) == n_glyph_ids + 1                      # unmapped glyph ids included
    assert cmd_off[0] == 0 and dat_off[0] == 0 and cmd_off[-1] == len(d["kinds"]) and dat_off[-1] == len(d["coords"])
    assert (np.diff(cmd_off) >= 0).all() and (np.diff(dat_off) >= 0).all()
    assert int(d["kinds"].max(initial=0)) <= 4
    run = np.concatenate([[0], np.cumsum(_n_floats(d["kinds"]))])
    assert np.array_equal(np.diff(dat_off), run[cmd_off[1:]] - run[cmd_off[:-1]])   # every glyph's range is what its kinds carry


def assert_names_the_recorded_outlines(vg, mgr, fid, n_glyph_ids=None):
    """-> (description, its records) of the font id's one file"""
    d = mgr.command_font_desc(fid, 0)
    if n_glyph_ids is None:
        n_glyph_ids = len(d["cmd_off"]) - 1
    assert_invariants(d, n_glyph_ids)
    records = expand(vg, d)
    r, o = mgr.record_resident_commands(fid), mgr.record_outlines(fid)
    for k in ("ids", "advances", "scale", "shift_x"):
        assert r[k].tobytes() == o[k].tobytes(), k
    assert r["n_files"] == 1 and (r["font_of"] == 0).all() and (r["glyph_id"] < n_glyph_ids).all()
    gid = r["glyph_id"].astype(np.int64)
    c0, c1 = d["cmd_off"].astype(np.int64)[gid], d["cmd_off"].astype(np.int64)[gid + 1]
    assert np.array_equal(np.concatenate([[0], np.cumsum(c1 - c0)]), o["cmd_off"].astype(np.int64))
    pick = np.concatenate([np.arange(a, b) for a, b in zip(c0, c1)]) if len(gid) else np.zeros(0, np.int64)
    got, want = records[pick], np.ascontiguousarray(o["cmds"])
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()          # every mapped code point's records, bit for bit
    return d, records


def test_fira_as_it_stands(vg):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Fira", [FIRA])
    d, _ = assert_names_the_recorded_outlines(vg, mgr, fid, TTFont(FIRA)["maxp"].numGlyphs)
    assert len(d["cmd_off"]) - 1 > 1686 and 3 in d["kinds"] or 2 in d["kinds"]    # more glyph ids than mapped code points
    # built once: the second description is the same table
    d2 = mgr.command_font_desc(fid, 0)
    assert all(np.array_equal(d[k], d2[k]) for k in d)


def test_fira_as_cff(vg, fira_as_cff):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Fira CFF", fira_as_cff)
    d, _ = assert_names_the_recorded_outlines(vg, mgr, fid, TTFont(io.BytesIO(fira_as_cff))["maxp"].numGlyphs)
    assert int((d["kinds"] == 3).sum()) > 1000 and len(mgr.record_resident_commands(fid)["ids"]) == 1686
    with pytest.raises(RuntimeError, match="glyf"):           # the glyf-resident calls still refuse the face
        mgr.resident_font_desc(fid, 0)
    with pytest.raises(RuntimeError, match="glyf"):
        mgr.record_resident(fid)


def test_the_synthetic_cff2_face(vg):
    from test_cff2_outlines import _NAMES
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("CFF2", _cff2())
    d, _ = assert_names_the_recorded_outlines(vg, mgr, fid, len(_NAMES))
    assert len(d["kinds"]) > 200          # (the "deep" glyph alone: 200 lines from its 400 operands)


def test_the_operator_and_subroutine_font(vg, ops_cff):  # noqa: F811
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Ops", ops_cff)
    d, _ = assert_names_the_recorded_outlines(vg, mgr, fid, 7)
    assert set(np.unique(d["kinds"])) >= {0, 1, 3, 4}


def _damage(font: bytes, rng, i: int) -> bytes:
    """tests/test_cff_outlines.py's damage (its child program): random bytes inside the CFF table — header / INDEX offsets /
    DICTs at its start, charstrings further in"""
    at = font.index(b"CFF ")
    off, ln = int.from_bytes(font[at + 8:at + 12], "big"), int.from_bytes(font[at + 12:at + 16], "big")
    b = bytearray(font)
    hi = (64, 600, ln)[i % 3]
    for pos in rng.integers(0, hi, int(rng.integers(1, 16))):
        b[off + int(pos)] = int(rng.integers(0, 256))
    return bytes(b)


@pytest.mark.parametrize("seed", [1, 2])
def test_damaged_cff_tables_agree_with_the_reader(vg, fira_as_cff, seed):
    """a charstring that fails midway leaves the callbacks delivered up to there — in the table as in a render"""
    clean = vg.FontManager(False)
    want = clean.command_font_desc(clean.add_font_data("Clean", fira_as_cff), 0)
    rng = np.random.default_rng(seed)
    n_loaded = n_differ = 0
    for i in range(1, 40):
        mutant = _damage(fira_as_cff, rng, i)
        mgr = vg.FontManager(False)
        try:
            fid = mgr.add_font_data(f"Mutant {i}", mutant)
        except RuntimeError:
            continue
        d, _ = assert_names_the_recorded_outlines(vg, mgr, fid)
        n_loaded += 1
        n_differ += not all(np.array_equal(d[k], want[k]) for k in d)
    print(f"seed {seed}: {n_loaded} mutants loaded, {n_differ} with other commands than the undamaged font")
    assert n_loaded >= 1 and n_differ >= 1


def test_refusals(vg):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Fira", [FIRA])
    with pytest.raises(RuntimeError):
        mgr.command_font_desc("no_such_font", 0)
    with pytest.raises(RuntimeError):
        mgr.command_font_desc(fid, 1)
    with pytest.raises(RuntimeError):
        mgr.command_font_desc(fid, -1)
    with pytest.raises(RuntimeError):
        mgr.record_resident_commands("no_such_font")


def test_a_table_past_32_bit_offsets_is_refused_without_allocating_it(vg):
    """1502 commands per leaf, 330 x 330 leaves under one glyph id: 163 million commands, a store of 4.7 GB (29 bytes each).  The
    callbacks are counted before anything is stored and the count ends at the bound, so the refusal costs no memory"""
    import resource
    from test_composite_fanout import fan_out_font
    # a modest fan-out is an ordinary table
    small = vg.FontManager(False)
    d, _ = assert_names_the_recorded_outlines(vg, small, small.add_font_data("Fan Small", fan_out_font(points=200, fan=3)), 4)
    assert list(np.diff(d["cmd_off"])) == [6, 202, 3 * 202, 9 * 202]
    big = vg.FontManager(False)
    fid = big.add_font_data("Fan Out", fan_out_font(points=1500, fan=330))
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    with pytest.raises(RuntimeError, match="32-bit"):
        big.command_font_desc(fid, 0)
    with pytest.raises(RuntimeError, match="32-bit"):
        big.record_resident_commands(fid)
    assert (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) / 1024 < 400


_C_PROGRAM = r"""
/* a plain C caller reads a command description and walks it (no device needed) */
#include <stdio.h>
#include "vgsdf.h"
#include "vgfont.h"
int main(int argc, char **argv)
{
	vg_manager *m = vg_manager_new(0);
	const char *files[1];
	vgsdf_font_cmds_desc d;
	vg_resident_batch *rb;
	vg_resident_view v;
	uint32_t g, c, n_cmds = 0;
	int (*create)(vgsdf_ctx *, const vgsdf_font_cmds_desc *, vgsdf_font **) = vgsdf_font_create_commands;
	if (argc < 2 || !m || !create)
		return 2;
	files[0] = argv[1];
	if (vg_manager_add_font_with_name(m, "Fira Sans Regular", files, 1) < 0 || vg_manager_command_font_desc(m, "fira_sans_regular", 0, &d) != 0) {
		fprintf(stderr, "desc: %s\n", vg_last_error());
		return 1;
	}
	if (d.cmd_off[0] != 0 || d.dat_off[0] != 0 || d.cmd_off[d.n_glyph_ids] != d.n_cmds || d.dat_off[d.n_glyph_ids] != d.n_floats)
		return 3;
	for (g = 0; g < d.n_glyph_ids; g++) {
		uint32_t floats = 0;
		for (c = d.cmd_off[g]; c < d.cmd_off[g + 1]; c++) {
			if (d.kinds[c] > 4)
				return 4;
			floats += d.kinds[c] <= 1 ? 2u : d.kinds[c] == 2 ? 4u : d.kinds[c] == 3 ? 6u : 0u;
		}
		if (d.dat_off[g + 1] - d.dat_off[g] != floats)
			return 5;
	}
	rb = vg_manager_record_resident_commands(m, "fira_sans_regular");
	if (!rb || vg_resident_batch_view(rb, &v) != 0 || v.n_files != 1 || v.n_glyphs < 1000 || v.ids[0] != 13)
		return 6;
	for (g = 0; g < v.n_glyphs; g++) {
		if (v.font_of[g] != 0 || v.glyph_id[g] >= d.n_glyph_ids)
			return 7;
		n_cmds += d.cmd_off[v.glyph_id[g] + 1] - d.cmd_off[v.glyph_id[g]];
	}
	if (vg_manager_command_font_desc(m, "no_such_font", 0, &d) == 0 || vg_manager_record_resident_commands(m, "no_such_font"))
		return 8;
	printf("%u glyphs name %u commands\n", (unsigned)v.n_glyphs, (unsigned)n_cmds);
	vg_resident_batch_free(rb);
	vg_manager_free(m);
	return 0;
}
"""


def test_the_new_declarations_are_plain_c(vg, tmp_path):
    """include/*.h still compile as C99 -pedantic -Werror; a plain C program reads a command description and walks it"""
    src = tmp_path / "commands.c"
    src.write_text(_C_PROGRAM)
    exe = tmp_path / "commands"
    lib = vg.lib_path()
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    f"-L{lib.parent}", f"-l:{lib.name}", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe), str(FIRA)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    # Fira: the 1686 mapped glyphs name the 45 943 commands the host's reader records for the font
    assert "1686 glyphs name 45943 commands" in p.stdout
