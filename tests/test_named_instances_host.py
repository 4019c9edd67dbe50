"""vg_manager_add_font_named_instances on the host: every instance record of a variable file's fvar becomes a font id of its own.

The ids are those of tests/named_instances_kit.py's restatement of the rule (which PostScript name an instance goes by, from
fontTools' reading of fvar and name); the coordinates are those vg_manager_add_font_instance arrives at for the record's location
(so normalisation and avar are that call's); what that call refuses is refused; vg_manager_scan and _add_path expand a file only
with vg_manager_set_scan_named_instances, and without it give the ids of today."""
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
import named_instances_kit as N  # noqa: E402
import variable_instances_kit as V  # noqa: E402
from conftest import FIRA  # noqa: E402


@pytest.mark.parametrize("which", ["shear", "scale_prefix", "two_axes_no_room", "edge"])
def test_ids_and_positions_of_every_record(vg, which):
    font, records = N.files()[which]
    want = N.instance_ids(vg, font)
    mgr = vg.FontManager(False)
    got = mgr.add_font_named_instances(font)
    assert got == want and len(got) == len(records)
    assert mgr.font_ids() == sorted(set(want))
    # two records of one id are two files of that id, in the table's order; every file is where add_font_instance puts it
    seen = {}
    for k, (fid, record) in enumerate(zip(got, records)):
        index = seen.get(fid, 0)
        seen[fid] = index + 1
        single = vg.FontManager(False)
        single.add_font_instance("Single", font, record["location"])
        assert list(mgr.font_position(fid, index)) == list(single.font_position("single")), (k, fid)
    assert max(seen.values()) == (2 if which in ("shear", "scale_prefix") else 1)


def test_the_postscript_name_decides_the_id():
    """the kit's files put the rule's branches side by side"""
    font, records = N.files()["shear"]
    family, names = N.ps_names(font)
    assert family == "Synth Gvar"
    assert names == ["SynthGvar-Medium", "SynthGvarRoman-SemiBold", "SynthGvar-Black", "SynthGvar-Black", "SynthGvar-", "SynthGvar-Regular"]
    assert N.ps_names(N.files()["scale_prefix"][0])[1] == ["SynthVF-Medium", "SynthGvarRoman-SemiBold", "SynthVF-Black", "SynthGvar-Black",
                                                          "SynthVF-", "SynthVF-Regular"]
    assert N.ps_names(N.files()["two_axes_no_room"][0])[1] == ["SynthGvar-Medium", "SynthGvar-ExtendedBold", "SynthGvar-ExtendedBlack"]


def test_a_cff2_file_with_avar_is_accepted(vg):
    base = V.variable_fira(avar={"wght": [(-1.0, -1.0), (0.0, 0.0), (0.5, 0.25), (1.0, 1.0)]})
    records = [dict(subfamily="Medium", ps=None, location={"wght": 525}), dict(subfamily="Bold", ps="Synth-Bold", location={"wght": 700})]
    font = N.with_instances(base, records)
    mgr = vg.FontManager(False)
    got = mgr.add_font_named_instances(font)
    assert got == N.instance_ids(vg, font) and len(set(got)) == 2
    for fid, record in zip(got, records):
        single = vg.FontManager(False)
        single.add_font_instance("Single", font, record["location"])
        assert list(mgr.font_position(fid)) == list(single.font_position("single")) == V.coords_of(font, record["location"])
        assert mgr.gvar_font_desc(fid) is None                                           # CFF2: the charstring path, no gvar


def test_what_is_refused(vg):
    mgr = vg.FontManager(False)
    with pytest.raises(RuntimeError, match="fvar"):
        mgr.add_font_named_instances(open(FIRA, "rb").read())
    with pytest.raises(RuntimeError, match="no instance record"):
        mgr.add_font_named_instances(N.no_instances(G.variable_glyf_fira("shear")))
    with pytest.raises(RuntimeError, match="no instance record"):
        mgr.add_font_named_instances(G.edge_faces()["inference"][0])
    # a glyf face without a readable gvar: add_font_instance's refusal, and nothing is added
    square = G.simple_entry([[(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]])
    without = N.with_instances(G.raw_font([square], None), N.EDGE, room_for_ps=False)
    with pytest.raises(RuntimeError, match="gvar"):
        mgr.add_font_named_instances(without)
    with pytest.raises(RuntimeError):
        mgr.add_font_named_instances(b"not a font")
    assert mgr.font_ids() == []
    # ... and a good file after them
    assert len(mgr.add_font_named_instances(N.files()["edge"][0])) == 4


def test_the_scan_switch(vg, tmp_path):
    font, _ = N.files()["shear"]
    (tmp_path / "fonts").mkdir()
    (tmp_path / "fonts" / "synth.ttf").write_bytes(font)
    (tmp_path / "fonts" / "static.ttf").write_bytes(open(FIRA, "rb").read())
    today = vg.FontManager(False)
    today.add_path(tmp_path / "fonts" / "synth.ttf")
    today.add_path(tmp_path / "fonts" / "static.ttf")
    for switch in (None, False):
        off = vg.FontManager(False)
        if switch is not None:
            off.set_scan_named_instances(switch)
        off.scan(tmp_path)
        assert off.font_ids() == today.font_ids() and len(off.font_ids()) == 2
        assert off.font_position(off.font_ids()[-1]) is None                          # at the default position, as the reference
    on = vg.FontManager(False)
    on.set_scan_named_instances(True)
    on.scan(tmp_path)
    static = [fid for fid in today.font_ids() if not fid.startswith("synth")]
    assert on.font_ids() == sorted(set(N.instance_ids(vg, font)) | set(static))
    by_path = vg.FontManager(False)
    by_path.set_scan_named_instances(True)
    by_path.add_path(tmp_path / "fonts" / "synth.ttf")
    assert by_path.font_ids() == sorted(set(N.instance_ids(vg, font)))
    # a variable file without instance records is added as ever
    (tmp_path / "bare").mkdir()
    (tmp_path / "bare" / "bare.ttf").write_bytes(N.no_instances(font))
    bare = vg.FontManager(False)
    bare.set_scan_named_instances(True)
    bare.scan(tmp_path / "bare")
    assert len(bare.font_ids()) == 1 and bare.font_position(bare.font_ids()[0]) is None
