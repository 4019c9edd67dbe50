"""The host half of device-built family tables (Face::family_tables, vg_manager_family_tables_desc), no GPU: the description
against fontTools' view of the fonts, and the Python restatement of a family (tests/cmap_edge_tables.py) over such
descriptions against the table the host reader builds (vg_manager_family_desc), element for element, doubles as bits.  The
edge tables are spliced into a fixture font with fontTools as raw tables."""
import io
import struct

import numpy as np
import pytest

import cmap_edge_tables as E
from conftest import FIRA, TESTDATA, noto_files

ttLib = pytest.importorskip("fontTools.ttLib")

KEYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")


def all_fixture_fonts():
    return [FIRA] + noto_files()


def _same_family(got, want):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


def test_21_fixtures(vg):
    assert len(all_fixture_fonts()) == 21


@pytest.mark.parametrize("path", all_fixture_fonts(), ids=lambda p: p.stem)
def test_description_equals_fonttools_view(vg, path):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("One", [path])
    d = mgr.family_tables_desc(fid, 0)
    assert d is not None
    ttf = ttLib.TTFont(str(path), lazy=True)
    cmap, hmtx = ttf.reader["cmap"], ttf.reader["hmtx"]
    assert d["cmap"] == cmap and d["hmtx"] == hmtx
    assert (d["units_per_em"], d["num_glyphs"], d["num_hmetrics"]) == (ttf["head"].unitsPerEm, ttf["maxp"].numGlyphs, ttf["hhea"].numberOfHMetrics)
    want = []
    for i in range(struct.unpack_from(">H", cmap, 2)[0]):          # the encoding records in the table's own order
        p, e, off = struct.unpack_from(">HHI", cmap, 4 + 8 * i)
        fmt = struct.unpack_from(">H", cmap, off)[0]
        if E.is_unicode(p, e, fmt) and fmt in E.FORMATS:
            want.append((off, fmt))
    by_tools = [(t.platformID, t.platEncID, t.format) for t in ttf["cmap"].tables]
    assert len(by_tools) == struct.unpack_from(">H", cmap, 2)[0]
    assert [f for p, e, f in by_tools if E.is_unicode(p, e, f) and f in E.FORMATS] == [f for _, f in want]
    assert list(zip(d["subtable_off"].tolist(), d["subtable_format"].tolist())) == want and len(want) >= 1
    # and the description is the Python one of the same tables
    mine = E.describe({"cmap": cmap, "hmtx": hmtx, "units_per_em": d["units_per_em"], "num_glyphs": d["num_glyphs"], "num_hmetrics": d["num_hmetrics"]})
    assert mine["subtable_off"].tolist() == d["subtable_off"].tolist() and mine["subtable_format"].tolist() == d["subtable_format"].tolist()


@pytest.mark.parametrize("which", ["fira", "noto_all"])
def test_restatement_equals_the_host_table_on_the_fixtures(vg, which):
    paths = [FIRA] if which == "fira" else noto_files()
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Font", paths)
    descs = [mgr.family_tables_desc(fid, k) for k in range(len(paths))]
    assert all(d is not None for d in descs)
    want = mgr.family_desc(fid)
    assert want["n_files"] == len(paths) and len(want["code_point"]) > 1000
    _same_family(E.restate(descs), want)
    assert 0xFFFF not in want["code_point"].tolist()               # the closing segment has a value there and lists nothing


def splice(face, base=FIRA):
    """the fixture font with the face's cmap and hmtx as raw tables and its three counts patched into head, maxp and hhea"""
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    ttf = ttLib.TTFont(str(base), lazy=True)
    raw = {tag: bytearray(ttf.reader[tag]) for tag in ("head", "maxp", "hhea")}
    struct.pack_into(">H", raw["head"], 18, face["units_per_em"])
    struct.pack_into(">H", raw["maxp"], 4, face["num_glyphs"])
    struct.pack_into(">H", raw["hhea"], 34, face["num_hmetrics"])
    raw["cmap"], raw["hmtx"] = face["cmap"], face["hmtx"]
    for tag, data in raw.items():
        t = DefaultTable(tag)
        t.data = bytes(data)
        ttf[tag] = t
    out = io.BytesIO()
    ttf.save(out)
    return out.getvalue()


def spliced_manager(vg, faces):
    mgr = vg.FontManager(False)
    for k, f in enumerate(faces):
        fid = mgr.add_font_data("Edge", splice(f))
    return mgr, fid


@pytest.mark.parametrize("name", sorted(E.regular_cases()) + ["past"])
def test_restatement_equals_the_host_table_on_the_edge_tables(vg, name):
    faces = E.past_case() if name == "past" else E.regular_cases()[name]
    mgr, fid = spliced_manager(vg, faces)
    descs = [mgr.family_tables_desc(fid, k) for k in range(len(faces))]
    for d, f in zip(descs, faces):
        mine = E.describe(f)
        assert d is not None and d["cmap"] == f["cmap"] and d["hmtx"] == f["hmtx"]
        assert (d["units_per_em"], d["num_glyphs"], d["num_hmetrics"]) == (f["units_per_em"], f["num_glyphs"], f["num_hmetrics"])
        assert d["subtable_off"].tolist() == mine["subtable_off"].tolist() and d["subtable_format"].tolist() == mine["subtable_format"].tolist()
    _same_family(E.restate(descs), mgr.family_desc(fid))


def test_edge_tables_hold_what_they_are_named_for():
    c = E.regular_cases()
    r = {k: E.restate([E.describe(f) for f in v]) for k, v in c.items()}
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        assert len(r[f"entries_{n}"]["code_point"]) == n
    assert r["special_code_points"]["code_point"].tolist() == [0, 0xD7FF, 0xE000, 0xFFFE]
    assert r["ffff_listed"]["code_point"][-1] == 0xFFFF and len(r["format4_1_segments"]["code_point"]) == 0
    two = r["two_subtables"]
    assert two["code_point"].tolist() == [0x41, 0x42, 0x43, 0xFFFF] and two["glyph_id"].tolist() == [4, 5, 6, 0]
    assert r["skipped_records"]["code_point"].tolist() == [0x44, 0x45]
    d = E.describe(c["skipped_records"][0])
    assert d["subtable_format"].tolist() == [4] and len(c["skipped_records"][0]["records"]) == 6
    ro = dict(zip(r["format4_range_offsets"]["code_point"].tolist(), r["format4_range_offsets"]["glyph_id"].tolist()))
    assert ro == {0x20: 4, 0x22: 5, 0x30: 5, 0x31: 6, 0x41: 7, 0x60: 9, 0x80: 11, 0xF070: E.SMALL[2], 0xF071: E.SMALL[2] + 1}
    assert r["varint_steps"]["advance"].tolist() == [127, 128, 127, 128] and r["varint_steps"]["pbf_fix"].tolist() == [0x22, 0x33, 0x23, 0x34]
    assert r["hmtx_all_metrics"]["advance"][:2].tolist() == [0, 1494] and set(r["hmtx_short"]["advance"].tolist()) == {0}
    assert r["hmtx_few_glyphs"]["advance"][4:].tolist() == [0] * 15 and len(set(r["hmtx_one_metric"]["advance"].tolist())) == 1
    assert set(r["faces_3"]["font_of"].tolist()) == {0, 1, 2} and set(r["middle_face_maps_nothing"]["font_of"].tolist()) == {0, 3}
    f12 = dict(zip(r["format12"]["code_point"].tolist(), r["format12"]["glyph_id"].tolist()))
    assert 0x100 not in f12 and 0x200 not in f12 and f12[0xFFFF] == 19 and f12[0x41] == 7


@pytest.mark.parametrize("name", sorted(E.irregular_cases()))
def test_irregular_tables_are_refused_and_the_host_table_still_answers(vg, name):
    mgr, fid = spliced_manager(vg, [E.irregular_cases()[name]])
    assert mgr.family_tables_desc(fid, 0) is None
    assert len(mgr.family_desc(fid)["code_point"]) >= 1
    with pytest.raises(RuntimeError):
        mgr.family_tables_desc(fid, 1)                                 # (a file index past the files is an error, not a refusal)


def test_every_fixture_font_is_regular(vg):
    for path in all_fixture_fonts():
        mgr = vg.FontManager(False)
        assert mgr.family_tables_desc(mgr.add_font_with_name("One", [path]), 0) is not None, path
    assert TESTDATA.exists()
