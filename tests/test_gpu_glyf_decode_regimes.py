"""The device's glyf decoder at its wave edges, in both stampings (glyf_decode: vgsdf_outlines_submit_glyf, and
glyf_decode_resident: vgsdf_outlines_submit_resident over a font made of the same entries).

The entries are the hand-written ones of tests/glyf_edge_entries.py (flag windows, coordinate windows, contour windows, the
limits from either side; tests/test_glyf_edge_entries_host.py proves their placement and pins the yardstick to the host's
reader).  The yardstick is the strict sequential decoder's callbacks, submitted as commands through outlines_prepare /
outlines_render: rects, seg_off, every segment's bytes and every bitmap of the device decoder must be equal — no tolerance.
Every batch runs by both routes to the context bytes: written by the decoder itself, and by the separate context pass (taken
when a glyph of the batch has a scale that is not positive and finite).  Refused entries (malformed, or beyond the decoder's
limits) fail their submission with VGSDF_E_GLYF and leave the context sound; only byte ranges and slots the C ABI admits are
handed to the device.
"""
import numpy as np
import pytest

import glyf_edge_entries as E

pytest.importorskip("fontTools")
pytestmark = pytest.mark.gpu

E_GLYF = -4   # vgsdf_status


def _transforms(rng, k):
    """the fuzz test's set: exact halves, random f32 values, a mirrored one"""
    if k % 3 == 0:
        t = [float(v) for v in rng.choice([0.5, 0.75, 1.0, -1.0, 1.25, 0.0], 4)]
    elif k % 3 == 1:
        t = [float(np.float32(v)) for v in rng.uniform(-1.5, 1.5, 4)]
    else:
        t = [-1.0, 0.0, 0.0, 1.0]
    return tuple(t) + (float(rng.integers(-300, 301)), float(rng.integers(-300, 301)))


def _forms(vg, glyphs, rng):
    """glyphs: [[(case, transform | None, extra slots), ...] per glyph] -> the glyf form, the description of a font with one glyph
    id per glyph (+ one without leaves), the yardstick's commands, scales and shifts"""
    from versatiles_glyphs_rs_amd.device import GLYF_PART_DTYPE, OUTLINE_CMD_DTYPE
    parts, leaves, data, store, stored = [], [], bytearray(), bytearray(), {}
    cmd_off, leaf_off, host_off, cmds, slots, scale = [0], [0], [0], [], 0, []
    for glyph in glyphs:
        ext, in_glyph = 0.0, 0
        for c, t, extra in glyph:
            p = np.zeros((), dtype=GLYF_PART_DTYPE)
            p["byte_off"], p["byte_len"] = len(data), len(c.part)
            p["cmd_at"], p["cmd_cap"], p["n_contours"] = slots, c.cmd_cap + extra, c.n_contours
            if t is None:
                p["plain"], p["a"], p["d"] = 1, 1.0, 1.0
            else:
                p["a"], p["b"], p["c"], p["d"], p["e"], p["f"] = t
            data += c.part + b"\0" * (-len(c.part) % 4)
            parts.append(p)
            lf = p.copy()
            if c.name not in stored:
                stored[c.name] = len(store)
                store += c.part + b"\0" * (-len(c.part) % 4)
            lf["byte_off"], lf["cmd_at"] = stored[c.name], in_glyph
            leaves.append(lf)
            slots += int(p["cmd_cap"])
            in_glyph += int(p["cmd_cap"])
            got = E.strict_decode(c.part, c.n_contours, int(p["cmd_cap"]), t)
            if isinstance(got, list):
                cmds += got
                ext = max([ext] + [abs(float(v)) for cb in got for v in cb[1:]])
        cmd_off.append(slots)
        leaf_off.append(len(leaves))
        host_off.append(len(cmds))
        scale.append(24.0 / 1000.0 if ext <= 1500.0 else 30.0 / ext)     # (entries all over the i16 range: keep the bitmaps small)
    leaf_off.append(len(leaves))                                            # the font's last glyph id has no leaves
    arr = np.zeros(len(cmds), dtype=OUTLINE_CMD_DTYPE)
    for k, (kind, x1, y1, x, y) in enumerate(cmds):
        arr[k]["kind"], arr[k]["x1"], arr[k]["y1"], arr[k]["x"], arr[k]["y"] = kind, x1, y1, x, y
    n = len(glyphs)
    return {
        "glyf": (np.array(cmd_off, np.uint32), np.array(parts, dtype=GLYF_PART_DTYPE), np.frombuffer(bytes(data), np.uint8)),
        "font": (np.array(leaf_off, np.uint32), np.array(leaves, dtype=GLYF_PART_DTYPE), np.frombuffer(bytes(store), np.uint8)),
        "host": (np.array(host_off, np.uint32), arr),
        "scale": np.array(scale, np.float64), "shift": rng.uniform(-0.5, 0.5, n), "n": n,
    }


def _yardstick(ctx, f):
    rects, out_bytes, n_seg = ctx.outlines_prepare(f["host"][0], f["host"][1], f["scale"], f["shift"])
    bitmaps = ctx.outlines_render()
    seg_off, segs = ctx.outlines_segments()
    return rects, bitmaps, int(out_bytes), seg_off, segs


def _submit(ctx, f, stamping, font, odd_scale):
    """one submission by the glyf form or over the resident font; odd_scale: one glyph without outline whose scale is not
    positive and finite is added, which sends the batch through the separate context pass"""
    n = f["n"]
    scale, shift = f["scale"], f["shift"]
    cmd_off, parts, data = f["glyf"]
    gids = np.arange(n)
    if odd_scale is not None:
        scale, shift = np.concatenate([scale, [odd_scale]]), np.concatenate([shift, [0.0]])
        cmd_off = np.concatenate([cmd_off, cmd_off[-1:]])
        gids = np.concatenate([gids, [n]])       # (the glyph id without leaves)
    if stamping == "glyf":
        ctx.outlines_submit_glyf(cmd_off, parts, data, scale, shift, capacity=f["capacity"])
    else:
        ctx.outlines_submit_resident([font], np.zeros(len(gids), np.uint16), gids, scale, shift, capacity=f["capacity"])


def _device(ctx, f, stamping, font, odd_scale=None):
    _submit(ctx, f, stamping, font, odd_scale)
    rects, bitmaps, out_bytes, n_seg = ctx.outlines_wait()
    seg_off, segs = ctx.outlines_segments()
    return rects, bitmaps, int(out_bytes), seg_off, segs


def _assert_equal(got, want, n, what):
    rects_d, bitmaps_d, ob_d, seg_off_d, segs_d = got
    rects_h, bitmaps_h, ob_h, seg_off_h, segs_h = want
    assert np.array_equal(rects_d[:n], rects_h), what
    assert np.array_equal(seg_off_d[:n + 1], seg_off_h), what
    assert segs_d.tobytes() == segs_h.tobytes(), what            # every segment, bit for bit
    assert ob_d == ob_h and bitmaps_d is not None and np.array_equal(bitmaps_d, bitmaps_h), what
    if len(rects_d) > n:   # the added glyph has nothing
        assert int(rects_d["n_segments"][n]) == 0 and int(rects_d["has_raster"][n]) == 0 and int(seg_off_d[n + 1]) == int(seg_off_d[n])


def _check_batch(vg, glyphs, seed, min_segments):
    rng = np.random.default_rng(seed)
    f = _forms(vg, glyphs, rng)
    ctx = vg.SdfContext(0)
    try:
        want = _yardstick(ctx, f)
        f["capacity"] = want[2] + 64
        font = ctx.font_create(*f["font"])
        for stamping in ("glyf", "resident"):
            _assert_equal(_device(ctx, f, stamping, font), want, f["n"], (stamping, "decoder writes cmd_open"))
            for odd in (0.0, -1.0, float("inf"), float("nan"))[seed % 2::2]:
                _assert_equal(_device(ctx, f, stamping, font, odd_scale=odd), want, f["n"], (stamping, "context pass", odd))
        font.free()
    finally:
        ctx.close()
    assert len(want[4]) >= min_segments
    return f, want


def _accepted(families):
    return [c for c in E.CASES if c.expect == E.ACCEPTED and c.family in families]


def _plain(cases):
    return [[(c, None, 0)] for c in cases]


def _moved(cases, seed):
    """every entry under two different transforms (and once plain, in between)"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k, c in enumerate(cases):
        out.append([(c, _transforms(rng, k), k % 3 if c.cmd_cap >= 64 else 0)])   # (some with filler slots)
        if c.n_points <= 2100:
            out.append([(c, _transforms(rng, k + 1), 0)])
        if k % 4 == 0:
            out.append([(c, None, 0)])
    return out


def test_the_restated_constants_are_the_kernels(vg):
    import ctypes as C
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    vg.load_library().vgsdf_glyf_limits(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (E.MAX_POINTS, E.MAX_BYTES, E.EXPAND_FONT_CACHE)


BATCHES = {
    "flag_windows": lambda: _accepted("A"),
    "coordinates": lambda: _accepted("B"),
    "contours": lambda: _accepted("C"),
    "limits": lambda: _accepted("D"),
    "lds_at_its_floor": lambda: [E.BY_NAME[n] for n in E.SMALL_CAP_BATCH],
    "one_6144_point_part_among_small_ones": lambda: [E.BY_NAME[n] for n in E.ONE_LARGE_AMONG_SMALL],
}


@pytest.mark.parametrize("moved", [False, True], ids=["plain", "transforms"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_accepted_entries_decode_to_the_strict_decoders_callbacks(vg, batch, moved):
    cases = BATCHES[batch]()
    assert len(cases) >= 5
    seed = list(BATCHES).index(batch)
    glyphs = _moved(cases, seed) if moved else _plain(cases)
    f, _ = _check_batch(vg, glyphs, seed, min_segments=50)
    caps = f["glyf"][1]["cmd_cap"]
    if batch == "lds_at_its_floor":
        assert int(caps.max()) < 64
    if batch == "one_6144_point_part_among_small_ones":
        assert np.sort(caps)[-1] >= E.MAX_POINTS and np.sort(caps)[-2] < 200


def test_glyphs_of_several_parts(vg):
    """2 to 4 edge entries per glyph: a part's filler slots, and a part whose last contour stays open, are followed by another part
    (its move_to, or the filler's close(), ends the ring); an open part also ends a glyph"""
    rng = np.random.default_rng(77)
    B = E.BY_NAME
    t = [_transforms(rng, k) for k in range(12)]
    glyphs = [
        [(B["C_open_end_smallest_cmd_cap"], None, 0), (B["A_repeat_lane63_w0_count08_nc1"], None, 0)],
        [(B["C_open_end_with_filler_slots"], t[0], 2), (B["C_finish_emits_two_quads_on_lane0"], None, 0),
         (B["C_open_end_last_point_on_lane0"], t[1], 0), (B["B_points_65"], t[2], 1)],
        [(B["D_cmd_cap_exact"], None, 5), (B["C_one_off_curve_point_contours_only"], None, 0), (B["A_flags_end_at_len_plain"], t[3], 0)],
        [(B["C_end_point_64_goes_back_into_window0"], t[4], 0), (B["C_open_end_last_point_on_lane63"], None, 0)],    # open at the glyph's end
        [(B["C_contours_65"], None, 0), (B["C_contours_65"], t[5], 3)],
        [(B["C_open_end_smallest_cmd_cap"], t[6], 0), (B["C_open_end_smallest_cmd_cap"], t[7], 0), (B["C_open_end_smallest_cmd_cap"], None, 0)],
        [(B["A_alternating_carry1_two_windows"], t[8], 0), (B["C_one_off_curve_point_then_a_contour"], None, 4),
         (B["C_off_curve_start_on_lane63_second_point_on_lane0"], t[9], 0), (B["B_x_sum_wraps_up_at_point_64"], t[10], 0)],
        [(B["C_end_point_64_equals_end_point_63"], None, 0), (B["D_points_6144"], t[11], 0)],
    ]
    assert {len(g) for g in glyphs} == {2, 3, 4}
    _check_batch(vg, glyphs, 5, min_segments=500)


REFUSED = [c for c in E.CASES if c.expect != E.ACCEPTED]


@pytest.mark.parametrize("name", [c.name for c in REFUSED])
def test_a_refused_entry_fails_its_submission_and_its_neighbour_passes(vg, name):
    bad = E.BY_NAME[name]
    k = [c.name for c in REFUSED].index(name)
    neighbour = E.BY_NAME[E.NEIGHBOURS[name]]
    if neighbour.expect != E.ACCEPTED:
        neighbour = E.BY_NAME[E.NEIGHBOURS[neighbour.name]]
    company = [E.BY_NAME[n] for n in ("D_cmd_cap_exact", "A_repeat_lane63_w0_count01_nc2", "C_contours_64", "B_points_129")]
    at = (0, 2, 4)[k % 3]                       # first, in the middle, last
    rng = np.random.default_rng(300 + k)

    def batch(c):
        cases = company[:at] + [c] + company[at:]
        return _forms(vg, [[(x, None if i % 2 else _transforms(rng, i), 0)] for i, x in enumerate(cases)], rng)

    f_bad, f_good = batch(bad), batch(neighbour)
    assert E.classify(bad.part, bad.n_contours, bad.cmd_cap) == bad.expect != E.ACCEPTED
    ctx = vg.SdfContext(0)
    try:
        want = _yardstick(ctx, f_good)
        f_bad["capacity"] = f_good["capacity"] = want[2] + (1 << 20)
        fonts = {"bad": ctx.font_create(*f_bad["font"]), "good": ctx.font_create(*f_good["font"])}
        for stamping in ("glyf", "resident"):
            for odd in (None, 0.0):
                _submit(ctx, f_bad, stamping, fonts["bad"], odd)
                with pytest.raises(vg.VgsdfError) as e:
                    ctx.outlines_wait()
                assert e.value.code == E_GLYF, (stamping, odd)
                # the next submission on the same context: the same batch with the accepted neighbour in the entry's place
                _assert_equal(_device(ctx, f_good, stamping, fonts["good"], odd), want, f_good["n"], (stamping, odd))
    finally:
        ctx.close()


def _render(vg, font, r, way):
    mgr = vg.FontManager(True)
    if way == "resident":
        mgr.set_resident_fonts(True)
    else:
        mgr.set_glyf_on_device(way == "device")
    mgr.add_font_data("Edge Entries", font)
    w = vg.DummyWriter()
    mgr.render_glyphs(w, r)
    return w.files, mgr.timings(), mgr.resident_stats()


def test_the_facade_writes_the_same_files_three_ways(vg):
    accepted = [c for c in E.CASES if c.expect == E.ACCEPTED]
    r = vg.Renderer.new_precise(0)
    font = E.font_with_entries([c.full for c in accepted])
    files = {}
    for way in ("device", "host", "resident"):
        files[way], t, s = _render(vg, font, r, way)
        assert t["glyf_fallbacks"] == 0 and t["glyphs"] == len(accepted)
        assert (t["glyf_groups"] >= 1) == (way == "device") and (s["groups"] >= 1) == (way == "resident")
    assert files["device"] == files["host"] == files["resident"] and len(files["host"]) >= 1
    # one entry beyond the decoder's limits among them: the group is recorded with the host's reader, once
    font = E.font_with_entries([c.full for c in accepted] + [E.BY_NAME["D_points_6145"].full])
    more = {}
    for way in ("device", "host", "resident"):
        more[way], t, _ = _render(vg, font, r, way)
        assert t["glyf_fallbacks"] == (0 if way == "host" else 1) and t["glyphs"] == len(accepted) + 1
    assert more["device"] == more["host"] == more["resident"] and more["host"] != files["host"]
