"""The device's builder of a placed `glyf` face's command store (vgsdf_font_create_gvar) against the host reader, which
tests/test_gvar_instances_host.py holds bit for bit against the kit's restatement of rules G1 to G6: for one face at one position
the command font the device builds from loca, glyf and gvar and the one vgsdf_font_create_commands makes of the reader's command
table are read back (vgsdf_font_commands_read) and compared byte for byte — cmd_off, the 28-byte records, the context bytes, and
what they occupy.

The faces: every hand-written table of tests/gvar_instances_kit.py at five positions (a face with a malformed glyph id at a
position must be refused there, and only there), glyph counts at the wave edges, the deltas budget at and one past it, the
validation of the description, the budget form at, under and over the store's size.  After every refusal a good call on the same
context succeeds."""
import struct

import numpy as np
import pytest

pytest.importorskip("fontTools")

import gvar_instances_kit as G  # noqa: E402

pytestmark = pytest.mark.gpu

VGSDF_E_ARG, VGSDF_E_GLYF = -1, -4
MAX_DELTAS = 1 << 20   # VGSDF_GVAR_MAX_DELTAS


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def _described(vg, font, coords):
    """(the description for the device, the host reader's command table) of `font` placed at the normalised coords"""
    mgr = vg.FontManager(False)
    fid = mgr.add_font_instance_normalized("Edge", font, coords)
    return mgr.gvar_font_desc(fid), mgr.command_font_desc(fid)


def assert_device_equals_host(ctx, desc, host):
    a = ctx.font_create_gvar(desc)
    b = ctx.font_create_commands(host["cmd_off"], host["dat_off"], host["kinds"], host["coords"])
    try:
        ra, rb = ctx.font_commands_read(a), ctx.font_commands_read(b)
        assert np.array_equal(rb["cmd_off"], host["cmd_off"])
        assert np.array_equal(ra["cmd_off"], rb["cmd_off"])
        assert ra["records"].tobytes() == rb["records"].tobytes()
        assert ra["context"].tobytes() == rb["context"].tobytes()
        assert a.device_bytes == b.device_bytes
    finally:
        a.free()
        b.free()


def refused(vg, ctx, code, desc, why, **override):
    with pytest.raises(vg.VgsdfError) as e:
        ctx.font_create_gvar(desc, **override)
    assert e.value.code == code and why in str(e.value), str(e.value)
    assert_device_equals_host(ctx, *_good(vg))       # the context is sound


GOOD = None


def _good(vg):
    global GOOD
    if GOOD is None:
        GOOD = _described(vg, G.edge_faces()["inference"][0], [16384])
    return GOOD


def _edge_coords(case, position):
    return position if case != "two_axes" else [position[0], -position[0] // 2 if position[0] > 0 else 16384]


def _at_five_positions(vg, ctx, case, font):
    """-> at how many of the positions the face was built"""
    built = 0
    for position in G.EDGE_POSITIONS:
        coords = _edge_coords(case, position)
        desc, host = _described(vg, font, coords)
        # a glyph id whose data is malformed AT THIS POSITION (a tuple of scalar 0 is not read) delivers nothing: the device refuses
        if all(G.restate(font, coords)["ok"]):
            assert_device_equals_host(ctx, desc, host)
            built += 1
        else:
            refused(vg, ctx, VGSDF_E_GLYF, desc, why="malformed variation data")
    return built


@pytest.mark.parametrize("case", sorted(G.edge_faces()))
def test_every_hand_written_face_at_five_positions(vg, ctx, case):
    font, malformed = G.edge_faces()[case]
    built = _at_five_positions(vg, ctx, case, font)
    # malformed whatever the tuples' scalars, so at every position: shared point numbers that descend, a shared tuple index
    # past the count, tuple headers cut short
    assert (built == 0) == (case in ("point_numbers_that_descend", "scalars", "truncated")), case
    # ... and with those glyph ids' tuple counts set to 0, the rest of such a face is built
    if built == 0 and case != "truncated":
        assert _at_five_positions(vg, ctx, case, _without_tuples(font, malformed)) >= 4


def _with_table(font, tag, change):
    """the font with table `tag` replaced by change(its bytes)"""
    import io
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    f = TTFont(io.BytesIO(font), recalcBBoxes=False, recalcTimestamp=False)
    t = DefaultTable(tag)
    t.data = bytes(change(bytearray(f.reader[tag])))
    f[tag] = t
    out = io.BytesIO()
    f.save(out)
    return out.getvalue()


def _without_tuples(font, glyph_ids):
    """the font with tupleVariationCount 0 for the glyph ids (long offsets)"""
    def change(data):
        data_at = struct.unpack(">I", data[16:20])[0]
        for g in glyph_ids:
            at = data_at + struct.unpack(">I", data[20 + 4 * g:24 + 4 * g])[0]
            data[at:at + 2] = b"\0\0"
        return data
    return _with_table(font, "gvar", change)


def _sized_face(n):
    """n glyph ids, unlike neighbours: simple glyphs of 4 to 67 points with subsets touched, every fifth a composite of two of them"""
    entries, datas = [], []
    for g in range(n):
        if g % 5 == 4:
            entries.append(G.composite_entry([(g - 1, 10 * g % 90, -7, None), (g - 3, -40, g % 50, (0.5, 0.25, -0.25, 0.75))]))
            datas.append(G.glyph_variations([G.tuple_of([24, -36, 0, 0, 0, 0], [12, 60 + g % 9, 0, 0, 0, 0], peak=[G.ONE], points=None)]))
        else:
            k = 4 + (g * 7) % 64
            entries.append(G.simple_entry([G._polygon(k, 1 + g % 3, (g, -g))]))
            numbers = list(range(g % 3, k, 2 + g % 4))
            datas.append(G.glyph_variations([G.tuple_of(G._ramp(len(numbers), 5 + g % 7), G._ramp(len(numbers), 3), peak=[G.ONE], points=numbers),
                                             G.tuple_of(G._ramp(k + 4, 11), G._ramp(k + 4, 13), peak=[G.HALF], inter=([0], [G.ONE]), points=None)]))
    return G.raw_font(entries, G.gvar_table(datas))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_glyph_counts_at_the_wave_edges(vg, ctx, n):
    font = _sized_face(n)
    for coords in ([16384], [5000]):
        desc, host = _described(vg, font, coords)
        assert len(host["cmd_off"]) == n + 1 and len(host["kinds"]) >= 6 * n
        assert_device_equals_host(ctx, desc, host)


def _budget_face(points):
    """glyph id 1: `points` points and 4095 tuples, all but the last on the negative side (scalar 0 at a positive position)"""
    n_all = points + 4
    last = G.pack_deltas(G._ramp(n_all)) + G.pack_deltas(G._ramp(n_all, 3))
    headers = struct.pack(">HHh", 0, 0x8000, -16384) * 4094 + struct.pack(">HHh", len(last), 0x8000, 16384)
    data = struct.pack(">HH", 4095, 4 + len(headers)) + headers + last
    square = G.simple_entry([[(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]])
    return G.raw_font([square, G.simple_entry([G._polygon(points)])], G.gvar_table([b"", data])), 4095 * n_all


def test_the_deltas_budget_at_and_one_past_it(vg, ctx):
    font, deltas = _budget_face(252)
    assert deltas <= MAX_DELTAS < deltas + 4095
    desc, host = _described(vg, font, [16384])
    assert_device_equals_host(ctx, desc, host)
    plain = vg.FontManager(False)
    assert host["coords"].tobytes() != plain.command_font_desc(plain.add_font_data("Edge", font))["coords"].tobytes()   # the last tuple moved it
    font, deltas = _budget_face(253)
    assert deltas > MAX_DELTAS
    refused(vg, ctx, VGSDF_E_GLYF, _described(vg, font, [16384])[0], why="VGSDF_GVAR_MAX_DELTAS")


def test_descriptions_that_are_refused(vg, ctx):
    desc, _ = _good(vg)
    gvar = desc["gvar"]
    array_end = 20 + 4 * (desc["num_glyphs"] + 1)
    for bad, why in ((dict(desc, gvar=b"\0\2" + gvar[2:]), "version"), (dict(desc, coords=[0, 0]), "axisCount"),
                     (dict(desc, coords=np.zeros(65, np.int16)), "1 .. 64"), (dict(desc, gvar=gvar[:19]), "header"),
                     (dict(desc, gvar=gvar[:array_end - 1]), "offset array"), (dict(desc, gvar=gvar[:array_end + 1]), "shared tuples"),
                     (dict(desc, loca_long=2), "loca_long"), (dict(desc, loca_entries=desc["loca_entries"] + 1), "loca entries"),
                     (dict(desc, num_glyphs=desc["num_glyphs"] - 1), "num_glyphs + 1")):
        refused(vg, ctx, VGSDF_E_ARG, bad, why=why)
    # the last glyph id's data leaves a gvar stated one byte shorter: malformed
    refused(vg, ctx, VGSDF_E_GLYF, desc, why="malformed variation data", gvar_len=len(gvar) - 1)


def test_a_glyf_length_shorter_than_the_table_bounds_every_read(vg, ctx):
    """the description states fewer glyf bytes than the uploaded table has: the device must build what the host reader makes of a
    file whose glyf table really ends there (an entry that leaves the table is no entry), not read on into the bytes behind"""
    font = G.edge_faces()["inference"][0]
    full, _ = _described(vg, font, [16384])
    n, stores = len(full["glyf"]), set()
    for cut in (1, 9, 40, n - 60, n - 11, n - 9):
        _, host = _described(vg, _with_table(font, "glyf", lambda data: data[:n - cut]), [16384])
        a = ctx.font_create_gvar(full, n_glyf_bytes=n - cut)
        b = ctx.font_create_commands(host["cmd_off"], host["dat_off"], host["kinds"], host["coords"])
        try:
            ra, rb = ctx.font_commands_read(a), ctx.font_commands_read(b)
            assert np.array_equal(ra["cmd_off"], rb["cmd_off"]), cut
            assert ra["records"].tobytes() == rb["records"].tobytes() and ra["context"].tobytes() == rb["context"].tobytes(), cut
            stores.add(len(ra["records"]))
        finally:
            a.free()
            b.free()
    _, whole = _good(vg)
    assert max(stores) < len(whole["kinds"]) and len(stores) >= 2          # the cuts took glyphs away


def _long_entry(n_points, n_contours):
    """a simple glyph of n_points in n_contours equal contours, in REPEAT flags and short coordinates (2 bytes a point): runs of
    256 points, x stepping by 0 or 1, y going up in one run and down in the next"""
    assert n_points % n_contours == 0 and n_points % 256 == 0
    ends = [(k + 1) * (n_points // n_contours) - 1 for k in range(n_contours)]
    e = struct.pack(">hhhhh", n_contours, 0, 0, 0, 0) + b"".join(struct.pack(">H", v) for v in ends) + b"\0\0"
    # ON_CURVE | X_SHORT | X_SAME (positive) | Y_SHORT | REPEAT, with Y_SAME (positive) in every other run
    e += b"".join(bytes([0x01 | 0x02 | 0x10 | 0x04 | 0x08 | (0x20 if r % 2 == 0 else 0), 255]) for r in range(n_points // 256))
    e += bytes(i % 2 for i in range(n_points)) + bytes(i % 5 for i in range(n_points))
    return e + b"\0" * (-len(e) % 2)


SLICE_POINTS = 1 << 17   # kGvarSlicePoints of csrc/gvar_limits.h


def _sliced_face(n_glyphs):
    """glyph ids whose own points (+ 4 phantom) fill more than one launch of the deltas pass: 0 a square, 1 - 3, 5 and 6 of 59904
    points, 4 a small glyph with a subset tuple, 7 a composite.  1, 3, 6 take one all-points tuple, 2 and 5 a subset (inference over
    contours of 19968 points).  Slices: [0, 3) of 119824 points, [3, 6) of 119828, [6, ...): glyph id 6 alone (n_glyphs 7) or with
    one more (8)"""
    big, n = _long_entry(59904, 3), 59904
    square = G.simple_entry([[(100, 100, True), (600, 100, True), (600, 600, True), (100, 600, True)]])
    small = G.simple_entry([G._polygon(12)])
    # (a tuple's data is at most 65535 bytes: two of three runs of 64 deltas are zero runs of one byte)
    sparse = lambda k: [v if (i // 64) % 3 == 0 else 0 for i, v in enumerate(G._ramp(n + 4, k))]  # noqa: E731
    every = lambda k: G.glyph_variations([G.tuple_of(sparse(k), sparse(k + 4), peak=[G.ONE], points=None)])  # noqa: E731
    def some(step):
        numbers = list(range(3, n, step))
        return G.glyph_variations([G.tuple_of(G._ramp(len(numbers), 5), G._ramp(len(numbers), 9), peak=[G.ONE], points=numbers)])
    entries = [square, big, big, big, small, big, big, G.composite_entry([(4, 100, 50, None), (0, -200, 0, (0.5, 0.25, -0.25, 0.75))])]
    datas = [G.glyph_variations([G.tuple_of([1, -2, 3, -4, 0, 0, 0, 0], [5, 6, -7, 8, 0, 0, 0, 0], peak=[G.ONE], points=None)]),
             every(7), some(7), every(11),
             G.glyph_variations([G.tuple_of([30, -10, 4], [8, 40, -4], peak=[G.ONE], points=[1, 6, 13])]), some(2001), every(13),
             G.glyph_variations([G.tuple_of([24, -36, 0, 0, 0, 0], [12, 60, 0, 0, 0, 0], peak=[G.ONE], points=None)])]
    own = [8, n + 4, n + 4, n + 4, 16, n + 4, n + 4, 6][:n_glyphs]
    assert sum(own[:3]) <= SLICE_POINTS < sum(own[:4]) and sum(own[3:6]) <= SLICE_POINTS < sum(own[3:7])
    return G.raw_font(entries[:n_glyphs], G.gvar_table(datas[:n_glyphs]))


@pytest.mark.parametrize("n_glyphs", [7, 8])
def test_glyph_ids_past_a_slice_of_the_deltas_pass(vg, ctx, n_glyphs):
    """three launches of the deltas pass over the context's scratch: the last is one glyph id alone, or that and one more"""
    desc, host = _described(vg, _sliced_face(n_glyphs), [16384])
    assert len(host["kinds"]) > 5 * 59904
    assert_device_equals_host(ctx, desc, host)
    plain = vg.FontManager(False)
    static = plain.command_font_desc(plain.add_font_data("Edge", _sliced_face(n_glyphs)))
    moved = [not np.array_equal(host["coords"][a:b], static["coords"][a:b]) for a, b in zip(host["dat_off"], host["dat_off"][1:])]
    assert all(moved)                                   # every glyph id took its deltas, in whichever slice it lay
    # a fresh context, whose scratch is grown by these very launches, gives the same store
    fresh = vg.SdfContext(0)
    try:
        assert_device_equals_host(fresh, desc, host)
        assert_device_equals_host(fresh, *_good(vg))
    finally:
        fresh.close()


def test_the_budget_form_at_under_and_over_the_store_size(vg, ctx):
    desc, host = _good(vg)
    none, want = ctx.font_create_gvar(desc, max_store_bytes=0)
    assert none is None and want == 29 * len(host["kinds"]) + 4 * len(host["cmd_off"])
    under, again = ctx.font_create_gvar(desc, max_store_bytes=want - 1)
    assert under is None and again == want
    f, again = ctx.font_create_gvar(desc, max_store_bytes=want)
    assert f is not None and again == want
    f.free()
    f, _ = ctx.font_create_gvar(desc, max_store_bytes=want + 1)
    assert f is not None
    f.free()
    assert_device_equals_host(ctx, desc, host)
    ms = ctx.font_gvar_kernel_ms()
    assert len(ms) == 3 and all(v > 0 for v in ms)
