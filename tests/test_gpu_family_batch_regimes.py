"""The family tables of ONE face at MANY positions in one device build (vgsdf_families_create_tables and its _mixed twin;
vgsdf_gvar_advance_deltas_batch: csrc/gvar_advance_batch_kernels.hip and the batched instantiations of csrc/family_table_kernels.hip).

The batched phantom pass is held to the host reader's Face::gvar_advance_delta (rule G7 of csrc/host/ttf_face.hpp), bit for bit
and at every position of one call, on the hand-written faces of tests/phantom_advances_kit.py and on faces padded around the
wave's edge in (glyph id, position) pairs.  Every family of a batched call is read back with vgsdf_family_read and compared, array
by array and byte for byte, with vgsdf_family_create over the reader's entries for that position.  No tolerance appears anywhere."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import family_batch_kit as B  # noqa: E402
from family_batch_kit import G, P, V  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_GLYF = B.E_ARG, B.E_GLYF


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


def _host_deltas(vg, font, positions):
    mgr = vg.FontManager(False)
    mgr.set_gvar_advances(True)
    fids = [mgr.add_font_instance_normalized(f"P{k}", font, list(p)) for k, p in enumerate(positions)]
    return mgr, mgr.gvar_font_desc(fids[0]), [mgr.font_gvar_advance_deltas(fid) for fid in fids]


def _pass_equals_host(vg, ctx, font, positions):
    mgr, desc, want = _host_deltas(vg, font, positions)
    got_d, got_state = ctx.gvar_advance_deltas_batch(desc, positions)
    assert got_d.shape == got_state.shape == (len(positions), int(desc["num_glyphs"]))
    for p, (want_d, want_state) in enumerate(want):
        assert got_state[p].tolist() == want_state.tolist(), p
        assert G.bits(got_d[p]) == G.bits(want_d), p
    return got_d, got_state


@pytest.mark.parametrize("case", sorted(P.faces()) + ["truncated"])
def test_the_pass_at_all_five_positions_in_one_call_equals_the_host_bit_for_bit(vg, ctx, case):
    font = P.truncated_face() if case == "truncated" else P.faces()[case][0]
    d, state = _pass_equals_host(vg, ctx, font, P.POSITIONS)
    assert ctx.families_tables_kernel_ms()[0] > 0 and ctx.families_tables_kernel_ms()[1:] == (0.0, 0.0)
    assert P.DELTA in set(state.ravel().tolist())
    # position [0] skips every tuple its neighbours in the wave read: no delta there, some at the others
    assert not d[0].any() and d[1:].any()
    if case in ("malformed", "truncated"):
        bad = state == P.MALFORMED                              # state 2 at some pairs and not at all of them
        assert bad.any() and not bad.all()
        if case == "malformed":                                 # a glyph id malformed where its tuple applies and not where it is skipped
            assert (bad.any(axis=0) & ~bad.all(axis=0)).any()


@pytest.mark.parametrize("n_ids,n_pos", [(1, 1), (1, 64), (64, 1), (21, 3), (22, 3), (43, 3), (65, 64)])
def test_the_pass_on_pairs_around_the_wave_edge(vg, ctx, n_ids, n_pos):
    cycle = ([0], [16384], [5000])
    positions = [cycle[k % 3] for k in range(n_pos)]
    assert n_ids * n_pos in (1, 64, 63, 66, 129, 4160)
    for at in sorted({0, n_ids - 1}):
        d, state = _pass_equals_host(vg, ctx, P.padded_face(n_ids, at), positions)
        others = np.arange(n_ids) != at
        assert not d[:, others].any() and not state[:, others].any()
        for p, pos in enumerate(positions):
            if pos == [16384]:
                assert d[p, at] == 59.0 + at and state[p, at] == P.DELTA
            if pos == [0]:
                assert d[p, at] == 0.0


def test_the_last_wave_of_one_lane(vg, ctx):
    # 65 glyph ids at one position, 13 at five: 65 pairs, the second wave holds the last glyph id alone
    for n_ids, positions in ((65, [[16384]]), (13, [[16384], [0], [5000], [16384], [8192]])):
        d, state = _pass_equals_host(vg, ctx, P.padded_face(n_ids, n_ids - 1), positions)
        assert n_ids * len(positions) == 65 and d[0, n_ids - 1] == 59.0 + n_ids - 1


@pytest.mark.parametrize("n_pos", [1, 3, 9])
@pytest.mark.parametrize("which", ["fira_without_hvar", "point_lists"])
def test_families_without_hvar_equal_the_readers_entries_at_every_position(vg, ctx, which, n_pos):
    fira = which == "fira_without_hvar"
    font = P.without_hvar("shear") if fira else P.faces()["point_lists"][0]
    positions = B.positions_with_a_twin(n_pos)
    placed = B.Placed(vg, ctx, font, positions, device_stores=fira)
    assert all(g is not None for g in placed.gvar) and not any(placed.variation)
    for mixed in (False, True):
        families, statuses = placed.batched(ctx, mixed=mixed)
        advances = B.assert_every_position(ctx, placed, families, statuses, mixed)
        ms = ctx.families_tables_kernel_ms()
        assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0
        if n_pos >= 3:
            assert len(set(advances)) >= 2                                   # at least two positions differ in advance
            assert advances[-1] == advances[0] and families[-1] is not families[0]   # the same position twice: two families
            families[0].free()
            B.assert_same(ctx, families[-1], placed.want(ctx, n_pos - 1, mixed), placed.entries[-1])   # each is freed alone
            families[0] = None
        B.free_all(families)


@pytest.mark.parametrize("n_pos", [1, 3, 9])
@pytest.mark.parametrize("which", ["glyf_fira", "cff2"])
def test_families_with_hvar_equal_the_readers_entries_and_the_phantom_pass_does_not_run(vg, ctx, which, n_pos):
    glyf = which == "glyf_fira"
    font = G.variable_glyf_fira("shear") if glyf else V.variable_fira(120)
    positions = B.positions_with_a_twin(n_pos)
    placed = B.Placed(vg, ctx, font, positions, device_stores=glyf)
    assert all(placed.variation) and placed.gvar == [None] * n_pos
    for mixed in (False, True):
        families, statuses = placed.batched(ctx, mixed=mixed)
        advances = B.assert_every_position(ctx, placed, families, statuses, mixed)
        ms = ctx.families_tables_kernel_ms()
        assert ms[0] == 0 and ms[1] > 0 and ms[2] > 0
        if n_pos >= 3:
            assert len(set(advances)) >= 2 and advances[-1] == advances[0]
        B.free_all(families)
    if glyf:    # with gvar given as well, HVAR still wins
        families, statuses = placed.batched(ctx, gvar=placed.mgr.gvar_font_desc(placed.fids[0]))
        B.assert_every_position(ctx, placed, families, statuses)
        assert ctx.families_tables_kernel_ms()[0] == 0
        B.free_all(families)
        # ... and without its records the same face takes gvar's deltas: the entries of the file without the table
        bare = B.Placed(vg, ctx, P.without_hvar("shear"), positions, device_stores=True)
        families, statuses = placed.batched(ctx, variation=None, gvar=placed.mgr.gvar_font_desc(placed.fids[0]))
        assert statuses == [0] * n_pos and ctx.families_tables_kernel_ms()[0] > 0
        for p, f in enumerate(families):
            assert ctx.family_read(f)["advance"].tobytes() == np.ascontiguousarray(bare.entries[p]["advance"]).tobytes()
        B.free_all(families)


def _sound(vg, ctx, placed):
    """a sound batched call and a sound single call on the same context"""
    families, statuses = placed.batched(ctx)
    B.assert_every_position(ctx, placed, families, statuses)
    B.free_all(families)
    single = ctx.family_create_tables_gvar([placed.stores[0]], [placed.tables[0]], [placed.variation[0]], [placed.gvar[0]])
    want = placed.want(ctx, 0)
    B.assert_same(ctx, single, want, placed.entries[0])
    single.free(), want.free()


def _refused(vg, call, code=E_ARG, sound=None):
    """the call is refused with `code`; sound: (ctx, placed) for a sound batched and a sound single call on the context behind it"""
    with pytest.raises(vg.VgsdfError) as e:
        call()
    assert e.value.code == code
    if sound:
        _sound(vg, *sound)
    return e.value


def test_refusals_leave_nothing_behind_and_the_context_sound(vg, ctx):
    font = P.faces()["point_lists"][0]
    placed = B.Placed(vg, ctx, font, [[16384], [5000], [0]])
    ok = (ctx, placed)
    for lie in ({"n_axes": 2}, {"gvar_len": 19}, {"n_axes": 0}, {"loca_entries": 4000}):
        _refused(vg, lambda: ctx.gvar_advance_deltas_batch(placed.gvar[0], placed.positions, **lie), sound=ok)
        _refused(vg, lambda: placed.batched(ctx, **lie), sound=ok)
    # NULL arguments, and a gvar description of another number of positions
    for null in ("desc", "fonts", "out", "status"):
        _refused(vg, lambda: placed.batched(ctx, null=[null]), sound=ok)
    _refused(vg, lambda: placed.batched(ctx, gvar_n_positions=2), sound=ok)
    _refused(vg, lambda: ctx.families_create_tables([placed.stores[0], None, placed.stores[2]], placed.face, None, placed.gvar[0], placed.positions),
             sound=ok)
    # 65 positions
    many = [[16384]] * 65
    _refused(vg, lambda: ctx.families_create_tables([placed.stores[0]] * 65, placed.face, None, placed.gvar[0], many), sound=ok)
    _refused(vg, lambda: ctx.gvar_advance_deltas_batch(placed.gvar[0], many), sound=ok)
    # none: VGSDF_OK, nothing is touched
    assert ctx.families_create_tables([], placed.face, None, placed.gvar[0], []) == ([], [])
    d, state = ctx.gvar_advance_deltas_batch(placed.gvar[0], [], n_axes=1)
    assert d.size == 0 and state.size == 0
    _sound(vg, ctx, placed)


def test_variation_records_that_do_not_name_one_hvar_are_refused(vg, ctx):
    placed = B.Placed(vg, ctx, V.variable_fira(120), [[8192], [16384], [5000]])
    ok = placed.variation
    n = len(ok[1]["hvar"])

    def sound():
        families, statuses = placed.batched(ctx)
        B.assert_every_position(ctx, placed, families, statuses)
        B.free_all(families)
        single = ctx.family_create_tables_var([placed.stores[1]], [placed.tables[1]], [ok[1]])
        want = placed.want(ctx, 1)
        B.assert_same(ctx, single, want, placed.entries[1])
        single.free(), want.free()

    def refused(call):     # (every refusal here: VGSDF_E_ARG, and the context sound behind it)
        with pytest.raises(vg.VgsdfError) as e:
            call()
        assert e.value.code == E_ARG
        sound()

    refused(lambda: placed.batched(ctx, variation=[ok[0], dict(ok[1], hvar_len=n - 1), ok[2]]))
    refused(lambda: placed.batched(ctx, variation=[ok[0], ok[1], dict(ok[2], hvar=bytes(ok[2]["hvar"]) + b"\0")]))
    refused(lambda: placed.batched(ctx, variation=[ok[0], dict(ok[1], map_off=ok[1]["map_off"] + 1), ok[2]]))
    refused(lambda: placed.batched(ctx, variation=[ok[0], ok[1], dict(ok[2], region_scalars=ok[2]["region_scalars"][:-1])]))
    refused(lambda: placed.batched(ctx, variation=[ok[0], None, ok[2]]))
    # what the single call refuses of a record: a factor that is not finite, at one position
    sc = ok[1]["region_scalars"].copy()
    sc[-1] = np.nan
    refused(lambda: placed.batched(ctx, variation=[ok[0], dict(ok[1], region_scalars=sc), ok[2]]))


def test_a_glyph_id_past_the_delta_budget_refuses_the_whole_call(vg, ctx):
    over = B.Placed(vg, ctx, P.over_budget_face(), [[16384], [0], [5000]])
    ok = (ctx, B.Placed(vg, ctx, P.faces()["point_lists"][0], [[16384], [5000]]))
    e = _refused(vg, lambda: over.batched(ctx), E_GLYF, sound=ok)        # (the binding asserts that every out[p] is NULL)
    assert "VGSDF_GVAR_MAX_DELTAS" in str(e)
    e = _refused(vg, lambda: ctx.gvar_advance_deltas_batch(over.gvar[0], over.positions), E_GLYF, sound=ok)
    assert "VGSDF_GVAR_MAX_DELTAS" in str(e)


@pytest.mark.parametrize("mixed", [False, True])
def test_a_font_of_fewer_glyph_ids_refuses_its_position_alone(vg, ctx, mixed):
    placed = B.Placed(vg, ctx, P.faces()["point_lists"][0], [[16384], [5000], [8192], [0]])
    short = B.Placed(vg, ctx, P.faces()["empty_entries"][0], [[5000]])      # 5 glyph ids against the face's 10
    stores = list(placed.stores)
    stores[1] = short.stores[0]
    families, statuses = ctx.families_create_tables(stores, placed.face, None, placed.gvar[0], placed.positions, mixed=mixed)
    assert statuses == [0, E_ARG, 0, 0] and families[1] is None
    assert "position 1" in ctx.last_error()
    for p in (0, 2, 3):
        want = placed.want(ctx, p, mixed)
        B.assert_same(ctx, families[p], want, placed.entries[p])
        want.free()
    B.free_all(families)
    # every position refused: the call is still VGSDF_OK
    families, statuses = ctx.families_create_tables([short.stores[0]] * 2, placed.face, None, placed.gvar[0], placed.positions[:2], mixed=mixed)
    assert statuses == [E_ARG, E_ARG] and families == [None, None]
    _sound(vg, ctx, placed)
