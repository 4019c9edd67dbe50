"""vg_manager_instance_group: the font ids of the faces that share one file's bytes — the group whose family tables
vg_manager_set_family_tables_batched builds in one device call.  Host only."""
import pytest

pytest.importorskip("fontTools")

import family_batch_kit as B  # noqa: E402
from conftest import FIRA  # noqa: E402
from family_batch_kit import G, NI, V  # noqa: E402


@pytest.mark.parametrize("which", ["shear", "two_axes_no_room", "edge"])
def test_the_group_of_a_named_instances_file_lists_all_its_records_ids(vg, which):
    font, records = NI.files()[which]
    mgr = vg.FontManager(False)
    ids = mgr.add_font_named_instances(font)
    assert ids == NI.instance_ids(vg, font) and len(ids) == len(records)
    alone = [i for i in ids if ids.count(i) == 1]
    assert len(alone) >= 2
    for font_id in alone:
        assert mgr.instance_group(font_id) == ids           # every record's id, in the table's order
    for font_id in set(ids) - set(alone):                   # two records arrive at one id: a font id of two files
        assert mgr.instance_group(font_id) == []
    assert (which == "shear") == bool(set(ids) - set(alone))


def test_cff2_instances_are_grouped_too(vg):
    base = V.variable_fira(40)
    records = [dict(subfamily="Medium", ps=None, location={"wght": 525}), dict(subfamily="Black", ps=None, location={"wght": 900})]
    font = NI.with_instances(base, records, room_for_ps=False)
    mgr = vg.FontManager(False)
    ids = mgr.add_font_named_instances(font)
    assert len(set(ids)) == 2 and mgr.instance_group(ids[0]) == ids and mgr.instance_group(ids[1]) == ids


def test_two_files_keep_their_own_groups_and_other_files_have_none(vg):
    mgr = vg.FontManager(False)
    a = mgr.add_font_named_instances(NI.files()["two_axes_no_room"][0])
    b = mgr.add_font_named_instances(NI.files()["edge"][0])
    assert not set(a) & set(b)
    assert mgr.instance_group(a[0]) == a and mgr.instance_group(b[-1]) == b
    static = mgr.add_font_data("Static", FIRA.read_bytes())
    placed = mgr.add_font_instance("Placed Alone", G.variable_glyf_fira("shear"), {"wght": 650})
    assert mgr.instance_group(static) == [] and mgr.instance_group(placed) == []
    assert mgr.instance_group("no_such_font") == []


def test_the_switch_and_its_stats_exist_and_start_at_nothing(vg):
    mgr = vg.FontManager(False)
    mgr.set_family_tables_batched(True)
    mgr.set_family_tables_batched(False)
    assert mgr.family_batch_stats() == {"calls": 0, "families": 0}
    assert B.positions_with_a_twin(3)[0] == B.positions_with_a_twin(3)[-1]
