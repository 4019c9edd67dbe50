"""The host half of a resident family (vg_manager_family_desc), no device needed: for a font id the table code point ->
(file, glyph id, advance, scale, shift_x) equals, element for element, the arrays a resident submission of every glyph of the id
names (vg_manager_record_resident; for a CFF face vg_manager_record_resident_commands).  Doubles are compared as bits; no
tolerance."""
import numpy as np
import pytest

from conftest import FIRA, NOTO, noto_files

PAIRS = (("font_of", "font_of"), ("glyph_id", "glyph_id"), ("scale", "scale"), ("shift_x", "shift_x"), ("code_point", "ids"),
         ("advance", "advances"))


def _assert_equals_the_recorded(d, r):
    assert d["n_files"] == r["n_files"] and len(d["code_point"]) == len(r["ids"]) > 0
    for mine, theirs in PAIRS:
        a, b = d[mine], r[theirs]
        assert len(a) == len(b) and a.astype(b.dtype).tobytes() == b.tobytes(), mine      # (doubles: bit for bit)
    assert d["scale"].dtype == np.float64 and d["shift_x"].dtype == np.float64
    assert (np.diff(d["code_point"].astype(np.int64)) > 0).all()                          # strictly ascending


@pytest.mark.parametrize("which", ["fira", "noto_regular", "noto_all"])
def test_the_table_equals_what_a_resident_submission_names(vg, which):
    paths = {"fira": [FIRA], "noto_regular": [NOTO]}.get(which) or noto_files()
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Font", paths)
    d = mgr.family_desc(fid)
    _assert_equals_the_recorded(d, mgr.record_resident(fid))
    _assert_equals_the_recorded(d, mgr.record_resident_commands(fid))       # the same table against either kind of store
    assert d["n_files"] == len(paths) == len(set(d["font_of"].tolist()))      # every file provides something
    # built once: the second view is the same table
    d2 = mgr.family_desc(fid)
    assert all(np.array_equal(d[k], d2[k]) for k in d if k != "n_files")


def test_a_cff_face(vg):
    pytest.importorskip("fontTools")
    from test_resident_commands_host import _cff2
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("CFF2", _cff2())
    _assert_equals_the_recorded(mgr.family_desc(fid), mgr.record_resident_commands(fid))
    with pytest.raises(RuntimeError, match="glyf"):            # (no glyf outlines: only command stores can back this family)
        mgr.record_resident(fid)


def test_the_table_is_rebuilt_when_a_file_is_added_to_the_id(vg):
    mgr = vg.FontManager(False)
    fid = mgr.add_font_with_name("Two", [FIRA])
    one = mgr.family_desc(fid)
    assert one["n_files"] == 1 and (one["font_of"] == 0).all()
    assert mgr.add_font_with_name("Two", [NOTO]) == fid
    two = mgr.family_desc(fid)
    _assert_equals_the_recorded(two, mgr.record_resident(fid))
    assert two["n_files"] == 2 and set(two["font_of"].tolist()) == {0, 1} and len(two["code_point"]) > len(one["code_point"])
    # first provider wins: what the first file maps stays with it
    first = np.isin(two["code_point"], one["code_point"])
    assert (two["font_of"][first] == 0).all() and np.array_equal(two["glyph_id"][first], one["glyph_id"])


def test_an_unknown_font_id(vg):
    mgr = vg.FontManager(False)
    with pytest.raises(RuntimeError, match="no_such_font"):
        mgr.family_desc("no_such_font")
