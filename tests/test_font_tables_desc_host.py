"""The host half of device-built glyf fonts (Face::font_tables, vg_manager_font_tables_desc), no GPU: the description against
fontTools' raw `loca` and `glyf`, and the Python restatement of the resident form (tests/composite_edge_trees.py) against the
table the host reader builds (Face::resident_table through vg_manager_resident_font_desc) — leaf_off equal, every leaf equal
except byte_off (the host stores entries in order of first encounter, the restatement in glyph-id order), the bytes every leaf
points at equal, the padding zero — on the 21 fixtures, on every edge font and on seeded damaged copies.  The restatement refuses
with its bounds exactly where the host's table is not ok."""
import subprocess

import numpy as np
import pytest

import composite_edge_trees as T
from conftest import FIRA, ROOT, noto_files

ttLib = pytest.importorskip("fontTools.ttLib")

FIELDS = [k for k in T.PART_DTYPE.names if k != "byte_off"]


def all_fixture_fonts():
    return [FIRA] + noto_files()


def tables_of(mgr, fid, k=0):
    d = mgr.font_tables_desc(fid, k)
    assert d is not None
    return T.Tables(d["loca"], d["glyf"], d["num_glyphs"], d["loca_entries"], d["loca_long"])


def host_table(mgr, fid, k=0):
    """the host's table, or None where it is not ok"""
    try:
        return mgr.resident_font_desc(fid, k)
    except RuntimeError:
        return None


def assert_same_content(mine, host):
    """the restated arrays against the host's table"""
    assert mine["leaf_off"].tobytes() == host["leaf_off"].tobytes()
    a, b = mine["leaves"], host["leaves"]
    assert len(a) == len(b)
    for k in FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k            # (floats as bits)
    mb, hb = mine["bytes"].tobytes(), host["bytes"].tobytes()
    assert len(mb) % 4 == 0 and len(hb) % 4 == 0
    seen = set()
    for m_off, h_off, ln in zip(a["byte_off"].tolist(), b["byte_off"].tolist(), a["byte_len"].tolist()):
        if (m_off, h_off) in seen:
            continue
        seen.add((m_off, h_off))
        padded = (ln + 3) & ~3
        assert m_off % 4 == 0 and m_off + padded <= len(mb)
        assert mb[m_off:m_off + padded] == hb[h_off:h_off + padded]
        assert mb[m_off + ln:m_off + padded] == b"\0" * (padded - ln)
    # the restated store is its glyph ids' entries back to back, and every leaf points at one
    at = mine["byte_at"]
    assert at[0] == 0 and at[-1] == len(mb) and (np.diff(at.astype(np.int64)) >= 0).all()
    assert set(a["byte_off"].tolist()) <= set(at[:-1].tolist())


def check_against_host(vg, t, font=None):
    """-> the restatement; asserted against the host's reading of the same tables"""
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Edge", T.font_of(t) if font is None else font)
    assert tables_of(mgr, fid) == t
    mine, host = T.restate(t), host_table(mgr, fid)
    if mine == T.REFUSED_BOUNDS:
        assert host is None
    elif mine == T.REFUSED_BUDGET:
        assert host is not None                                # (the host reader has no budget: the device's refusal is its own)
    else:
        assert host is not None
        assert_same_content(mine, host)
    return mine


def test_21_fixtures():
    assert len(all_fixture_fonts()) == 21


@pytest.mark.parametrize("path", all_fixture_fonts(), ids=lambda p: p.stem)
def test_fixture_description_equals_fonttools_and_restatement_equals_the_host_table(vg, path):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("One", [path])
    t = tables_of(mgr, fid)
    ttf = ttLib.TTFont(str(path), lazy=True)
    assert t.loca == ttf.reader["loca"] and t.glyf == ttf.reader["glyf"]
    n, long = ttf["maxp"].numGlyphs, ttf["head"].indexToLocFormat
    assert (t.num_glyphs, t.loca_long) == (n, long) and t.loca_entries == min(n + 1, len(t.loca) // (4 if long else 2))
    mine = T.restate(t)
    assert_same_content(mine, mgr.resident_font_desc(fid))
    assert len(mine["leaves"]) >= n // 2


@pytest.mark.parametrize("name", T.LONG_CASES)
def test_edge_case_alone(vg, name):
    check_against_host(vg, T.case_tables(name))


@pytest.mark.parametrize("order", [1, -1])
def test_edge_cases_side_by_side(vg, order):
    mine = check_against_host(vg, T.forest_of(T.LONG_CASES, order).tables())
    assert len(mine["leaves"]) > 900


@pytest.mark.parametrize("name", sorted(T.LOCA_FONTS))
def test_loca_fonts(vg, name):
    t = T.LOCA_FONTS[name]
    if name in ("no_loca", "no_glyf"):          # not a glyf face: the manager takes no such file; the restatement has nothing to say
        mine = T.restate(t)
        assert len(mine["leaves"]) == 0 and len(mine["bytes"]) == 0 and mine["leaf_off"].tolist() == [0] * (t.num_glyphs + 1)
        return
    check_against_host(vg, t)


def test_edge_fonts_hold_what_they_are_named_for():
    def leaves_of(name, glyph=None):
        f = T.forest_of([name])
        r = T.restate(f.tables())
        g = f.gid(glyph or name)
        return r["leaves"][r["leaf_off"][g]:r["leaf_off"][g + 1]], r["records"][g]
    a, b = "leafA", "leafB"
    f = T.forest_of(["args_words"])
    at = T.restate(f.tables())["byte_at"]
    A, B = int(at[f.gid(a)]), int(at[f.gid(b)])
    lv, _ = leaves_of("args_words")
    assert lv["byte_off"].tolist() == [A, B] and (lv["e"].tolist(), lv["f"].tolist()) == ([300.0, -32768.0], [-200.0, 32767.0]) and lv["plain"].tolist() == [0, 0]
    lv, _ = leaves_of("args_bytes_negative")
    assert (lv["e"].tolist(), lv["f"].tolist()) == ([-5.0, 127.0], [-128.0, -1.0])
    lv, _ = leaves_of("args_xy_bytes_consumed_neighbour")
    assert lv["byte_off"].tolist() == [A, B] and lv["e"].tolist() == [0.0, 7.0]
    lv, n = leaves_of("args_anchor_bytes_not_consumed")          # the point numbers are read as the next record
    assert lv["byte_off"].tolist()[:1] == [A] and lv["plain"][0] == 1 and n > 2
    lv, _ = leaves_of("args_anchor_words_with_scale")
    assert lv["a"].tolist() == [0.5] and lv["e"].tolist() == [0.0]       # 0x2000 read as the scale
    lv, _ = leaves_of("args_xy_words_with_scale_neighbour")
    assert lv["a"].tolist() == [0.5] and lv["e"].tolist() == [8192.0]
    lv, _ = leaves_of("scale_all_three_bits")
    assert lv["b"][0] != 0 and lv["c"][0] != 0 and len(lv) == 2           # the 2x2 is read, the record behind it is found
    lv, _ = leaves_of("scale_xy_over_uniform")
    assert lv["a"][0] != lv["d"][0] and lv["b"][0] == 0 and len(lv) == 2
    lv, _ = leaves_of("f2dot14_extremes")
    assert lv["a"][0] == -2.0 and lv["d"][0] == np.float32(32767) / np.float32(16384)
    for name, levels in (("compose_two_levels", 2), ("compose_three_levels", 3)):
        lv, _ = leaves_of(name)
        assert len(lv) == levels + 1
        # the deepest leaf's transform is not what f64 arithmetic rounds to: the f32 order matters
        deep = lv[-1]
        assert all(np.isfinite(float(deep[k])) for k in "abcdef") and deep["plain"] == 0
    for form in ("words", "bytes", "scale", "xy_scale", "two_by_two"):
        assert len(leaves_of(f"truncated_{form}_whole")[0]) == 2
        for cut in ("last_byte_missing", "header_only", "header_three_bytes"):
            lv, n = leaves_of(f"truncated_{form}_{cut}")
            assert len(lv) == 1 and n == (1 if cut == "header_three_bytes" else 2), (form, cut)
    for name in ("child_ffff", "child_past_loca", "child_empty_range", "child_no_contours_two_bytes", "child_no_contours_with_body"):
        lv, n = leaves_of(name)
        assert lv["byte_off"].tolist() == [B] and n == 2, name
    for name in ("child_lone_point", "child_instructions_to_the_end"):
        assert len(leaves_of(name)[0]) == (2 if name == "child_lone_point" else 3), name
    for name in ("child_no_contours_one_byte_fails", "child_simple_header_nine_bytes", "child_composite_header_nine_bytes",
                 "child_last_end_ffff_fails_in_the_middle", "child_end_points_past_the_entry", "child_no_instruction_length",
                 "child_instructions_past_the_entry"):
        lv, n = leaves_of(name)
        assert lv["byte_off"].tolist() == [A] and n == 2, name            # the leaf in front stays, the one behind is not reached
    assert len(leaves_of("child_composite_header_only")[0]) == 2          # an empty composite succeeds
    lv, _ = leaves_of("child_entry_of_32k")
    assert lv["byte_len"].tolist()[1] == T.MAX_ENTRY and len(lv) == 3
    lv, _ = leaves_of("child_entry_past_32k")
    assert lv["byte_len"].tolist()[1] == 0 and len(lv) == 3
    assert len(leaves_of("no_more_components_with_bytes_behind")[0]) == 1
    lv, n = leaves_of("chain_depth_31")
    assert len(lv) == 32 and lv["byte_off"].tolist()[-1] == B and n == 62
    for name in ("chain_depth_32", "chain_depth_33"):
        lv, n = leaves_of(name)
        assert len(lv) == 31 and set(lv["byte_off"].tolist()) == {A} and n == 63   # leafA at depth 32 fails the glyph
    lv, n = leaves_of("names_itself")
    assert len(lv) == 31 and n == 63
    lv, _ = leaves_of("cycle_of_two_with_a_leaf_in_front")
    assert len(lv) >= 1 and lv["byte_off"][0] == B
    assert len(leaves_of("glyph_of_600_leaves")[0]) == 600
    # loca
    whole, cut = T.restate(T.LOCA_FONTS["range_whole_neighbour"]), T.restate(T.LOCA_FONTS["range_past_glyf"])
    assert len(whole["leaves"]) == 2 + 3 + 1 and len(cut["leaves"]) == 2 + 2
    assert any(int.from_bytes(T.LOCA_FONTS["short_loca_odd_offsets"].loca[2 * i:2 * i + 2], "big") % 2 for i in range(4))
    a, b = T.restate(T.LOCA_FONTS["short_loca"]), T.restate(T.LOCA_FONTS["short_loca_odd_offsets"])
    assert a["leaves"].tobytes() == b["leaves"].tobytes()
    shared = T.restate(T.LOCA_FONTS["two_glyph_ids_share_a_range"])
    assert len(shared["bytes"]) == len(a["bytes"]) + 16 and shared["leaf_off"][-1] - shared["leaf_off"][-2] == 1
    # the bounds
    at, past = T.restate(T.budget_font(0)), T.restate(T.budget_font(1))
    assert max(at["records"]) == T.MAX_COMPONENTS and len(at["leaves"]) == 2 and past == T.REFUSED_BUDGET
    at, past = T.restate(T.slots_font(1023)), T.restate(T.slots_font(1024))
    assert int(at["slots"].max()) == 1023 * 65537 <= T.MAX_GLYPH_SLOTS < 1024 * 65537 and past == T.REFUSED_BOUNDS
    at, past = T.restate(T.leaves_font(0)), T.restate(T.leaves_font(1))
    assert len(at["leaves"]) == T.MAX_LEAVES == int(at["leaf_off"][-1]) and past == T.REFUSED_BOUNDS
    assert max(at["records"]) < T.MAX_COMPONENTS


def test_the_bounds_against_the_host(vg):
    for t in (T.budget_font(0), T.budget_font(1), T.slots_font(1023), T.slots_font(1024), T.leaves_font(0), T.leaves_font(1)):
        check_against_host(vg, t)


def test_the_replay_of_the_restatement_changes_nothing(monkeypatch):
    """the restatement replays a subtree it has walked where every transform is a shift by whole numbers; walked record by record
    instead (the shifts made too large to qualify), the same fonts give the same arrays"""
    fonts = [T.case_tables("glyph_of_600_leaves"), T.forest_of(T.LONG_CASES).tables(), T.LOCA_FONTS["short_loca"], T.count_font(129, 64)]
    with_replay = [T.restate(t) for t in fonts]
    monkeypatch.setattr(T, "_WHOLE", 0)
    monkeypatch.setattr(T, "_RESTATED", {})
    for t, a in zip(fonts, with_replay):
        b = T.restate(t)
        for k in ("leaf_off", "leaves", "bytes", "slots"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["records"] == b["records"]


@pytest.mark.parametrize("n,deep_at,kind", [(1, None, "mixed"), (63, None, "mixed"), (64, 0, "mixed"), (65, 63, "mixed"), (127, 64, "mixed"),
                                            (128, 127, "mixed"), (129, 128, "mixed"), (65, None, "simple"), (65, None, "composite")])
def test_count_fonts(vg, n, deep_at, kind):
    mine = check_against_host(vg, T.count_font(n, deep_at, kind))
    if deep_at is not None:
        assert mine["leaf_off"][deep_at + 1] - mine["leaf_off"][deep_at] == 32       # 31 links' leaves and the leaf at depth 31
    if kind == "composite":
        assert len(mine["leaves"]) == 0 and len(mine["bytes"]) == 0


def damaged(t, rng, i):
    """a copy of the tables damaged the i-th way: loca entries, component flags, child ids, truncations"""
    loca, glyf = bytearray(t.loca), bytearray(t.glyf)
    size = 4 if t.loca_long else 2
    way = i % 6
    if way == 0:                                                          # a loca entry: anywhere, also past glyf
        k = int(rng.integers(0, len(loca) // size))
        loca[k * size:(k + 1) * size] = int(rng.choice([0, 2, len(glyf) // (1 if t.loca_long else 2), int(rng.integers(0, len(glyf) + 9)) // (1 if t.loca_long else 2),
                                                        (1 << (8 * size)) - 1])).to_bytes(size, "big")
    elif way == 1:                                                        # glyf truncated
        glyf = glyf[:int(rng.integers(1, len(glyf)))]
    elif way == 2:                                                        # loca truncated (the entry count follows the bytes)
        loca = loca[:int(rng.integers(size, len(loca)))]
    else:                                                                 # bytes of glyf: flags, child ids, headers, arguments
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(0, len(glyf)))
            glyf[at] = int(rng.choice([0, 0x20, 0x21, 0x23, 0x28, 0x60, 0xA3, 0xFF, int(rng.integers(0, 256))])) if way < 5 else (glyf[at] ^ (1 << int(rng.integers(0, 8))))
    want = 0xFFFF if t.num_glyphs == 0xFFFF else t.num_glyphs + 1
    return T.Tables(bytes(loca), bytes(glyf), t.num_glyphs, min(want, len(loca) // size), t.loca_long)


def mutants():
    """-> [(name, Tables)]: 300 seeded damaged copies of three edge fonts"""
    bases = [T.forest_of(T.LONG_CASES[:30]).tables(), T.forest_of(T.LONG_CASES[30:], -1).tables(), T.LOCA_FONTS["short_loca"]]
    rng = np.random.default_rng(11)
    return [(f"mutant_{b}_{i}", damaged(base, rng, i)) for b, base in enumerate(bases) for i in range(100)]


def test_damaged_copies(vg):
    refused = 0
    for name, t in mutants():
        refused += isinstance(check_against_host(vg, t), str)
    print(refused, "of 300 refused")


_C_PROGRAM = r"""
/* a plain C caller states a face by its tables (no device needed) */
#include <stdio.h>
#include "vgsdf.h"
#include "vgfont.h"
int main(int argc, char **argv)
{
	vg_manager *m = vg_manager_new(0);
	const char *files[1];
	vgsdf_font_tables_desc d;
	vgsdf_font_desc host;
	int (*create)(vgsdf_ctx *, const vgsdf_font_tables_desc *, vgsdf_font **) = vgsdf_font_create_tables;
	int (*within)(vgsdf_ctx *, const vgsdf_font_tables_desc *, uint64_t, vgsdf_font **, uint64_t *) = vgsdf_font_create_tables_within;
	int (*read)(vgsdf_ctx *, const vgsdf_font *, uint32_t *, uint32_t *, uint32_t *, uint32_t *, vgsdf_glyf_part *, uint8_t *) = vgsdf_font_read;
	void (*ms)(const vgsdf_ctx *, float[2]) = vgsdf_font_tables_kernel_ms;
	if (argc < 2 || !m || !create || !within || !read || !ms)
		return 2;
	files[0] = argv[1];
	if (vg_manager_add_font_with_name(m, "Fira Sans Regular", files, 1) < 0 || vg_manager_font_tables_desc(m, "fira_sans_regular", 0, &d) != 0 ||
	    vg_manager_resident_font_desc(m, "fira_sans_regular", 0, &host) != 0) {
		fprintf(stderr, "desc: %s\n", vg_last_error());
		return 1;
	}
	if (d.num_glyphs != host.n_glyph_ids || d.loca_entries != d.num_glyphs + 1 || d.loca_long > 1 || !d.loca || !d.glyf ||
	    d.n_loca_bytes < d.loca_entries * (d.loca_long ? 4u : 2u))
		return 3;
	if (vg_manager_font_tables_desc(m, "no_such_font", 0, &d) == 0 || vg_manager_font_tables_desc(m, "fira_sans_regular", 1, &d) == 0)
		return 4;
	printf("%u glyph ids, %u loca bytes, %u glyf bytes\n", (unsigned)d.num_glyphs, (unsigned)d.n_loca_bytes, (unsigned)d.n_glyf_bytes);
	vg_manager_free(m);
	return 0;
}
"""


def test_the_new_declarations_are_plain_c(vg, tmp_path):
    """include/*.h still compile as C99 -pedantic -Werror; a plain C program asks for a face's tables"""
    src = tmp_path / "tables.c"
    src.write_text(_C_PROGRAM)
    exe = tmp_path / "tables"
    lib = vg.lib_path()
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    f"-L{lib.parent}", f"-l:{lib.name}", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe), str(FIRA)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    ttf = ttLib.TTFont(str(FIRA), lazy=True)
    assert f"{ttf['maxp'].numGlyphs} glyph ids, {len(ttf.reader['loca'])} loca bytes, {len(ttf.reader['glyf'])} glyf bytes" in p.stdout


def test_a_face_without_glyf_outlines_is_refused(vg):
    from fira_cff_kit import fira_as_cff
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Cff", fira_as_cff(60))
    assert mgr.font_tables_desc(fid, 0) is None
    with pytest.raises(RuntimeError):
        mgr.font_tables_desc(fid, 1)
