"""The edge entries of tests/glyf_edge_entries.py on the CPU: every case sits where it claims to sit (`roles`), the strict
sequential decoder and the host's reader (csrc/host/ttf_face.cpp) agree on every entry's class and on every callback of the
accepted ones bit for bit, `record_glyf_parts` lists the entries' bytes as they were written, and the resident form expands
to the same parts.  The device decoder is held against the strict decoder in tests/test_gpu_glyf_decode_regimes.py.
"""
import numpy as np
import pytest

import glyf_edge_entries as E
from test_resident_font_host import assert_expands_to_the_glyf_form

pytest.importorskip("fontTools")

f32 = np.float32
NAMES = [c.name for c in E.CASES]


def test_the_enumeration_is_complete():
    counts = E.family_counts()
    for fam, (n, a, m, d) in counts.items():
        print(f"family {fam}: {n} cases ({a} accepted, {m} malformed, {d} beyond the device's limits)")
    # what the families are asked to hold at least (flag windows, coordinates, contours, limits as pairs)
    assert counts["A"][0] >= 55 and counts["B"][0] >= 22 and counts["C"][0] >= 25 and counts["D"][0] >= 24
    assert all(c.check is not None for c in E.CASES) and len(set(NAMES)) == len(NAMES)
    assert set(E.NEIGHBOURS) == {c.name for c in E.CASES if c.expect != E.ACCEPTED}
    assert all(E.BY_NAME[v].expect == E.ACCEPTED or k == "D_last_end_point_fffe" for k, v in E.NEIGHBOURS.items())
    assert len(E.SMALL_CAP_BATCH) >= 8 and max(E.BY_NAME[n].cmd_cap for n in E.SMALL_CAP_BATCH) < 64
    assert sorted(E.BY_NAME[n].n_points for n in E.ONE_LARGE_AMONG_SMALL)[-2:][0] < 64 and E.BY_NAME["D_points_6144"].n_points == E.MAX_POINTS


def test_the_restated_constants_are_the_kernels(vg):
    import ctypes as C
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    vg.load_library().vgsdf_glyf_limits(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (E.MAX_POINTS, E.MAX_BYTES, E.EXPAND_FONT_CACHE) == (6144, 30 * 1024, 128)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_sits_where_it_claims_to_sit(name):
    c = E.BY_NAME[name]
    lay = E.layout(c.part, c.n_contours)
    c.check(c, lay)
    assert E.classify(c.part, c.n_contours, c.cmd_cap) == c.expect
    r = E.roles(c.part, c.n_contours)
    assert len(r) == max(len(c.part) - 2 * c.n_contours, 0) and all(lane == s % 64 for s, (_, lane) in enumerate(r))
    if lay.why is None:
        # flags and counts lie in front of x_at, everything from there on is behind the needed flags
        assert all(role != "behind" for role, _ in r[:lay.x_at - 2 * c.n_contours]) and all(role == "behind" for role, _ in r[lay.x_at - 2 * c.n_contours:])
    got = E.strict_decode(c.part, c.n_contours, c.cmd_cap)
    assert (got == c.expect) if c.expect != E.ACCEPTED else (isinstance(got, list) and len(got) <= c.cmd_cap)
    if c.expect == E.ACCEPTED and c.n_points > 1:
        assert len(got) >= 1
    # the full entry is the part with the header and an empty instruction array put in
    nc2 = 2 * c.n_contours
    if len(c.part) >= nc2:
        assert c.full[:2] == c.n_contours.to_bytes(2, "big") and c.full[10:10 + nc2] == c.part[:nc2] and c.full[12 + nc2:] == c.part[nc2:]


@pytest.fixture(scope="module")
def recorded(vg):
    font = E.font_with_entries([c.full for c in E.CASES])
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Edge Entries", font)
    o, g = mgr.record_outlines(fid), mgr.record_glyf_parts(fid)
    assert list(o["ids"]) == [0x100 + i for i in range(len(E.CASES))] == list(g["ids"])
    first = np.searchsorted(g["parts"]["cmd_at"], g["cmd_off"].astype(np.int64)[:-1], side="left")
    last = np.searchsorted(g["parts"]["cmd_at"], g["cmd_off"].astype(np.int64)[1:], side="left")
    return mgr, fid, o, g, first, last


def _host_callbacks(o, gi):
    return [(int(c["kind"]), f32(c["x1"]), f32(c["y1"]), f32(c["x"]), f32(c["y"])) for c in o["cmds"][o["cmd_off"][gi]:o["cmd_off"][gi + 1]]]


@pytest.mark.parametrize("name", NAMES)
def test_the_strict_decoder_and_the_host_reader_agree_on_class_and_callbacks(recorded, name):
    _, _, o, _, _, _ = recorded
    gi = NAMES.index(name)
    c = E.CASES[gi]
    want = _host_callbacks(o, gi)
    if c.expect == E.MALFORMED:
        assert want == []                                    # ttf-parser returns None: no outline
        return
    # accepted, or well-formed and beyond the device (the host's reader records the full outline)
    got = E.decode_callbacks(c.part, c.n_contours)
    assert len(got) == len(want) and len(got) >= 1
    if c.expect == E.ACCEPTED:
        assert len(got) <= c.cmd_cap
    for a, b in zip(got, want):
        assert a[0] == b[0] and all(x.tobytes() == y.tobytes() or (x == 0 and y == 0) for x, y in zip(a[1:], b[1:])), name


@pytest.mark.parametrize("name", NAMES)
def test_record_glyf_parts_lists_the_entries_as_written(recorded, name):
    _, _, _, g, first, last = recorded
    gi = NAMES.index(name)
    c = E.CASES[gi]
    parts = g["parts"][first[gi]:last[gi]]
    if not c.in_font:
        assert len(parts) == 0 and g["cmd_off"][gi] == g["cmd_off"][gi + 1]   # refused before anything is listed
        return
    assert len(parts) == 1
    p = parts[0]
    off, ln = int(p["byte_off"]), int(p["byte_len"])
    assert off % 4 == 0 and g["bytes"][off:off + ln].tobytes() == c.part
    assert int(p["n_contours"]) == c.n_contours and int(p["cmd_cap"]) == c.n_points + 2 * c.n_contours and int(p["plain"]) == 1
    assert int(p["cmd_at"]) == int(g["cmd_off"][gi]) and int(g["cmd_off"][gi + 1]) - int(g["cmd_off"][gi]) == int(p["cmd_cap"])


def test_the_resident_form_expands_to_the_same_parts(recorded):
    mgr, fid, _, g, _, _ = recorded
    _, r, descs = assert_expands_to_the_glyf_form(mgr, fid)
    assert r["n_files"] == 1 and len(r["glyph_id"]) == len(E.CASES)
    assert list(r["glyph_id"]) == [i + 1 for i in range(len(E.CASES))]     # one glyph id per entry
    assert len(descs[0]["leaves"]) == 1 + sum(c.in_font for c in E.CASES)     # (.notdef's square is a leaf too)
