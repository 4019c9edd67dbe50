"""The phantom pass on the device (csrc/gvar_advance_kernels.hip: vgsdf_gvar_advance_deltas) and the family tables that use it
(vgsdf_family_create_tables_gvar and its _mixed twin; the fourth instantiation of the emit pass in csrc/family_table_kernels.hip).

The pass is held to the host reader's Face::gvar_advance_delta (rule G7 of csrc/host/ttf_face.hpp), bit for bit, on the
hand-written faces of tests/phantom_advances_kit.py at their five positions and on faces padded around the wave's edge; the host
reader itself is held to the kit's restatement by tests/test_phantom_advances_host.py.  The families are read back with
vgsdf_family_read and compared, array by array and byte for byte, with vgsdf_family_create over the reader's entries.  No
tolerance appears anywhere."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402
import phantom_advances_kit as P  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_GLYF = -1, -4
ARRAYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "cmd_pre", "leaf_pre", "pbf_fix")
ENTRY_KEYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


def _placed(vg, font, coords, on=True):
    mgr = vg.FontManager(False)
    mgr.set_gvar_advances(on)
    return mgr, mgr.add_font_instance_normalized("P", font, coords)


def _pass_equals_host(vg, ctx, font, coords, extra=0):
    mgr, fid = _placed(vg, font, coords)
    desc = mgr.gvar_font_desc(fid)
    want_d, want_state = mgr.font_gvar_advance_deltas(fid)
    got_d, got_state = ctx.gvar_advance_deltas(desc)
    assert got_state.tolist() == want_state.tolist()
    assert G.bits(got_d) == G.bits(want_d)
    return got_d, got_state


@pytest.mark.parametrize("case", sorted(P.faces()) + ["truncated"])
def test_the_pass_equals_the_host_bit_for_bit_on_every_hand_written_face(vg, ctx, case):
    font = P.truncated_face() if case == "truncated" else P.faces()[case][0]
    states = set()
    for position in P.POSITIONS:
        d, state = _pass_equals_host(vg, ctx, font, position)
        states |= set(state.tolist())
        assert ctx.gvar_advance_kernel_ms() > 0
    assert P.DELTA in states
    if case in ("malformed", "truncated"):
        assert P.MALFORMED in states


@pytest.mark.parametrize("n_ids", [1, 63, 64, 65, 129])
def test_the_pass_on_faces_padded_around_the_wave_edge(vg, ctx, n_ids):
    for at in sorted({0, n_ids - 1, min(63, n_ids - 1), min(64, n_ids - 1)}):
        font = P.padded_face(n_ids, at)
        d, state = _pass_equals_host(vg, ctx, font, [16384])
        assert len(d) == n_ids and d[at] == 59.0 + at and state[at] == P.DELTA
        assert not d[np.arange(n_ids) != at].any() and not state[np.arange(n_ids) != at].any()


class Family:
    """the files of ONE font id in one manager (which owns the bytes the descriptions point into), their device fonts and their
    descriptions; add: (font bytes, coords or None)"""

    def __init__(self, vg, ctx, files, on=True):
        self.mgr = vg.FontManager(False)
        self.mgr.set_gvar_advances(on)
        for font, coords in files:
            self.fid = self.mgr.add_font_data("P", font) if coords is None else self.mgr.add_font_instance_normalized("P", font, coords)
        n = len(files)
        self.stores = []
        for k in range(n):
            d = self.mgr.command_font_desc(self.fid, k)
            self.stores.append(ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"]))
        self.tables = [self.mgr.family_tables_desc(self.fid, k) for k in range(n)]
        self.variation = [self.mgr.family_variation_desc(self.fid, k) for k in range(n)]
        self.gvar = [self.mgr.family_gvar_desc(self.fid, k) for k in range(n)]
        self.entries = self.mgr.family_desc(self.fid)

    def want(self, ctx, mixed=False):
        make = ctx.family_create_mixed if mixed else ctx.family_create
        return make(self.stores, *[self.entries[k] for k in ENTRY_KEYS])


def assert_same(ctx, got, want, entries):
    a, b = ctx.family_read(got), ctx.family_read(want)
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for k in ENTRY_KEYS:
        assert a[k].tobytes() == np.ascontiguousarray(entries[k]).tobytes(), k
    assert got.device_bytes == want.device_bytes and got.count(0, 0xFFFF) == len(entries["code_point"])


@pytest.mark.parametrize("case", sorted(P.faces()))
def test_a_family_of_one_hand_written_face_equals_the_readers_entries(vg, ctx, case):
    font = P.faces()[case][0]
    moved = 0
    for position in ([16384], [5000]):
        fam = Family(vg, ctx, [(font, position)])
        assert fam.gvar[0] is not None and not fam.variation[0]
        got, want = ctx.family_create_tables_gvar(fam.stores, fam.tables, fam.variation, fam.gvar), fam.want(ctx)
        assert_same(ctx, got, want, fam.entries)
        assert ctx.gvar_advance_kernel_ms() > 0
        off = Family(vg, ctx, [(font, position)], on=False)
        moved += off.entries["advance"].tobytes() != fam.entries["advance"].tobytes()
        got.free(), want.free()
    assert moved


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
@pytest.mark.parametrize("mixed", [False, True])
def test_a_family_of_a_static_an_hvar_and_a_gvar_face_in_one_call(vg, ctx, order, mixed):
    with_hvar, without = G.variable_glyf_fira("shear"), P.without_hvar("shear")
    files = [(P.faces()["point_lists"][0], None), (with_hvar, [8192]), (without, [8192])]
    fam = Family(vg, ctx, [files[i] for i in order])
    kinds = [("static", "hvar", "gvar")[i] for i in order]
    assert [bool(v) for v in fam.variation] == [k == "hvar" for k in kinds]
    assert [g is not None for g in fam.gvar] == [k == "gvar" for k in kinds]
    got, want = ctx.family_create_tables_gvar(fam.stores, fam.tables, fam.variation, fam.gvar, mixed=mixed), fam.want(ctx, mixed)
    assert_same(ctx, got, want, fam.entries)
    assert len(set(fam.entries["font_of"].tolist())) >= 2
    got.free(), want.free()


def test_hvar_wins_over_a_gvar_description_and_no_array_is_the_var_call(vg, ctx):
    font = G.variable_glyf_fira("shear")
    fam = Family(vg, ctx, [(font, [8192])])
    assert fam.gvar == [None] and fam.variation[0]
    both = [fam.mgr.gvar_font_desc(fam.fid, 0)]                    # the face's tables, although its advances do not follow them
    got, want = ctx.family_create_tables_gvar(fam.stores, fam.tables, fam.variation, both), fam.want(ctx)
    assert_same(ctx, got, want, fam.entries)
    assert ctx.gvar_advance_kernel_ms() == 0                        # (the pass did not run)
    plain = ctx.family_create_tables_gvar(fam.stores, fam.tables, fam.variation, None)
    var = ctx.family_create_tables_var(fam.stores, fam.tables, fam.variation)
    assert_same(ctx, plain, var, fam.entries)
    # without its HVAR record the same face takes gvar's deltas: the entries of the file without the table
    bare = Family(vg, ctx, [(P.without_hvar("shear"), [8192])])
    moved = ctx.family_create_tables_gvar(fam.stores, fam.tables, None, both)
    assert ctx.family_read(moved)["advance"].tobytes() == np.ascontiguousarray(bare.entries["advance"]).tobytes()
    for f in (got, want, plain, var, moved):
        f.free()


def test_refusals_leave_nothing_behind_and_the_context_sound(vg, ctx):
    font = P.faces()["point_lists"][0]
    fam = Family(vg, ctx, [(font, [16384])])
    desc = fam.gvar[0]
    for lie in ({"n_axes": 2}, {"gvar_len": 19}, {"n_axes": 0}, {"loca_entries": 4000}):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.gvar_advance_deltas(desc, **lie)
        assert e.value.code == E_ARG, lie
        with pytest.raises(vg.VgsdfError) as e:
            ctx.family_create_tables_gvar(fam.stores, fam.tables, fam.variation, fam.gvar, **lie)
        assert e.value.code == E_ARG, lie
    # over the budget by tuple count x points, with a few bytes of data: refused by the count
    big = P.over_budget_face()
    over = Family(vg, ctx, [(big, [16384])])
    with pytest.raises(vg.VgsdfError) as e:
        ctx.gvar_advance_deltas(over.gvar[0])
    assert e.value.code == E_GLYF and "VGSDF_GVAR_MAX_DELTAS" in str(e.value)
    with pytest.raises(vg.VgsdfError) as e:
        ctx.family_create_tables_gvar(over.stores, over.tables, over.variation, over.gvar)
    assert e.value.code == E_GLYF
    # ... and the next calls on the context are sound
    got, want = ctx.family_create_tables_gvar(fam.stores, fam.tables, fam.variation, fam.gvar), fam.want(ctx)
    assert_same(ctx, got, want, fam.entries)
    _pass_equals_host(vg, ctx, font, [16384])
    got.free(), want.free()
