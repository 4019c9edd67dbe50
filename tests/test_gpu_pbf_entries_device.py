"""pbf_entries (csrc/outline_plan_kernels.hip): the bytes of every glyph's PBF entry around its bitmap, written on the device behind
the plan of a ranges submission with pbf_pre.  Command fonts of axis-aligned rectangles at scale 1 make every field of an entry
the test's to choose — a rectangle (X, Y, W, H) has width W, height H, left X, top Y + H - 24 and a bitmap of (W + 6)(H + 6)
bytes — and the family gives every glyph its id (the code point) and advance.  Per task the arena's bytes behind the reserved
room are compared with the entries part of vg_pbf_encode's output for the rects and bitmaps read back: byte equality, every
varint edge asserted to occur.  The reserved rooms and every bitmap byte are compared with a vgsdf_outlines_submit_resident run
over an arena filled with the same pattern."""
import numpy as np
import pytest

import family_ranges_kit as K

pytestmark = pytest.mark.gpu

MOVE, LINE, CLOSE = 0, 1, 4
FILL = 0xA5
CAPACITY = 4 << 20
ID_EDGES = [0, 127, 128, 16383, 16384, 65535]
ADVANCE_EDGES = [0, 127, 128, 16383, 16384, 1 << 21, 1 << 28, (1 << 32) - 1]
FIELD_EDGES = [-65, -64, -1, 0, 63, 64]                 # left and top: zigzag 129, 127, 1, 0, 126, 128
MSG_EDGES = [127, 128, 16383, 16384]


def _msg_len(W, H, cp, adv):
    zz = lambda v: ((v << 1) ^ (v >> 31)) & 0xFFFFFFFF  # noqa: E731
    px = (W + 6) * (H + 6)
    return (1 + K.varint_len(cp) + 1 + K.varint_len(px) + px + 4 + K.varint_len(W) + K.varint_len(H) + K.varint_len(zz(0)) +
            K.varint_len(zz(H - 24)) + 1 + K.varint_len(adv))


def _cases():
    """-> [(code point, advance, X, Y, W, H)]; W = 0: a glyph id without outline"""
    cases = []
    for j, cp in enumerate(ID_EDGES):                   # ids, each with an advance edge; some without a raster
        cases.append((cp, ADVANCE_EDGES[j], 2, 3, 10 + j, 12, ))
    cases.append((1, 5, 0, 0, 0, 0))                     # without raster: one-byte id ...
    cases.append((129, 16384, 0, 0, 0, 0))               # ... two-byte id, three-byte advance
    cases.append((16385, (1 << 32) - 1, 0, 0, 0, 0))     # ... three-byte id, five-byte advance
    cp = 200
    for adv in ADVANCE_EDGES:                            # every advance edge on a rasterised glyph
        cases.append((cp, adv, 1, 1, 9, 9))
        cp += 1
    for W, H in ((127, 20), (128, 20), (20, 127), (20, 128), (1, 12), (2, 10), (121, 123), (122, 122)):
        cases.append((cp, 600, 4, 30, W, H))             # width / height fields at 127 | 128; w h at 126, 128, 16383, 16384
        cp += 1
    for v in FIELD_EDGES:
        cases.append((cp, 7, v, 5, 11, 13))              # left
        cases.append((cp + 1, 7, 5, v + 24 - 13, 11, 13))   # top = Y + H - 24
        cp += 2
    # message lengths either side of a varint step, by search over small rectangles (ids and advances fixed per search)
    found = {}
    for want in MSG_EDGES:
        for adv in (3, 300, 70000, 1 << 22, 1 << 30):
            for W in range(1, 260):
                for H in range(1, 260):
                    if want not in found and _msg_len(W, H, cp, adv) == want:
                        found[want] = (cp, adv, 0, 0, W, H)
    assert sorted(found) == MSG_EDGES
    for want in MSG_EDGES:
        c = found[want]
        cases.append((cp,) + c[1:])
        cp += 1
    for j in range(300):                                 # more than a workgroup of glyphs, and a raster of many spans
        cases.append((20000 + j, 40 + j, j % 7, j % 5, 60, 60))
    cases.sort()
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def _font(vg, cases):
    """glyph id i = the rectangle of case i: move, three lines, close (none for W = 0) -> the arrays of font_create_commands"""
    from versatiles_glyphs_rs_amd.device import OUTLINE_CMD_DTYPE
    cmds, cmd_off = [], [0]
    for _, _, X, Y, W, H in cases:
        if W:
            c = np.zeros(5, dtype=OUTLINE_CMD_DTYPE)
            c["kind"] = [MOVE, LINE, LINE, LINE, CLOSE]
            c["x"][:4] = [X, X + W, X + W, X]
            c["y"][:4] = [Y, Y, Y + H, Y + H]
            cmds.append(c)
        cmd_off.append(cmd_off[-1] + (5 if W else 0))
    cmd_off = np.array(cmd_off, np.uint32)
    dat_off, kinds, coords = vg.SdfContext.pack_outlines(cmd_off, np.concatenate(cmds))
    return cmd_off, dat_off, kinds, coords


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture()
def dev(vg, cases):
    ctx = vg.SdfContext(0)
    try:
        font = ctx.font_create_commands(*_font(vg, cases))
        n = len(cases)
        kit = type("Kit", (), {"ctx": ctx, "kinds": [font]})()
        # scale 1 and no shift where the test chooses the fields; every other filler at half the size and two pixels to the right
        scale, shift = np.ones(n), np.zeros(n)
        odd = np.array([c[0] >= 20000 and c[0] % 2 == 1 for c in cases])
        scale[odd], shift[odd] = 0.5, 2.0
        fam = K.Family(kit, [0], [c[0] for c in cases], np.zeros(n, int), np.arange(n), [c[1] for c in cases], scale, shift)
        yield ctx, fam
    finally:
        ctx.close()


TASKS = [(0, 0, 127, 30), (0, 128, 16383, 0), (0, 16384, 19999, 31), (0, 20000, 20299, 5), (0, 20300, 65535, 200),
         (0, 300, 310, 9), (0, 1, 1, 17), (0, 129, 129, 0)]      # (the last three: no glyph; one glyph without a raster, with and without room)


def _expected_entries(vg, rects, arena, at, ids, adv):
    """the entries part of vg_pbf_encode's output for these glyphs (name and range empty: 4 bytes of fields behind the length)"""
    glyphs = []
    for r, a, i, d in zip(rects, at, ids, adv):
        has = bool(r["has_raster"])
        w, h = int(r["w"]), int(r["h"])
        g = vg.PbfGlyph(id=int(i), has_bitmap=int(has), width=w - 6 if has else 0, height=h - 6 if has else 0,
                        left=int(r["x0"]) + 3 if has else 0, top=int(r["y0"]) + h - 27 if has else 0, advance=int(d))
        if has:
            g.bitmap = arena[int(a):int(a) + w * h].reshape(h, w)
        glyphs.append(g)
    blob = np.frombuffer(vg.pbf_encode("", "", glyphs), np.uint8)
    skip = 1
    while blob[skip] & 0x80:
        skip += 1
    skip += 1
    assert blob[0] == 0x0A and blob[skip:skip + 4].tolist() == [0x0A, 0, 0x12, 0]
    return blob[skip + 4:]


def _check_arena(vg, fam, tasks, rects, arena, at, begin, direct=True):
    """direct: the raster and the entries stored through the caller's page-locked arena itself (else the arena is a copy of the
    device's, rooms and all, as in every other form)"""
    args, pbf, ids, adv, first_glyph = K.sequence([fam], tasks, True)
    counts = [fam.handle.count(t[1], t[2]) for t in tasks]
    g = 0
    for t, n in enumerate(counts):
        lo, hi = int(begin[t]), int(begin[t + 1])
        if n == 0:
            assert lo == hi
            continue
        room = tasks[t][3]
        assert not direct or (arena[lo:lo + room] == FILL).all()       # the reserved room is the caller's
        want = _expected_entries(vg, rects[g:g + n], arena, at[g:g + n], ids[g:g + n], adv[g:g + n])
        assert arena[lo + room:hi].tobytes() == want.tobytes(), f"task {t}"
        g += n
    assert g == len(rects) and int(begin[-1]) == len(arena)


def _run(ctx, fam, tasks, capacity=CAPACITY, pinned=True, expect_in_place=None):
    fo, first, last, room = [np.array([t[i] for t in tasks], np.int64) for i in range(4)]
    ctx.outlines_submit_ranges([fam.handle], fo, first, last, capacity=capacity, pbf_pre=room, fill=FILL, pinned=pinned)
    if expect_in_place is not None:
        assert ctx.outlines_peek()[2] == expect_in_place
    rects, arena, out_bytes, _ = ctx.outlines_wait()
    if arena is None:                                                    # the arena did not fit: rendered on request
        assert out_bytes > capacity
        arena = ctx.outlines_render()
    return rects, arena, ctx.outlines_pbf_positions(), ctx.outlines_task_extents()


def test_every_varint_edge_occurs(vg, dev, cases):
    ctx, fam = dev
    rects, arena, at, begin = _run(ctx, fam, [(0, 0, 65535, 0)])
    by_cp = {c[0]: r for c, r in zip(cases, rects)}
    has = rects["has_raster"] != 0
    assert all(cp in by_cp for cp in ID_EDGES) and set(ADVANCE_EDGES) <= {c[1] for c in cases}
    assert {127, 128} <= set((rects["w"][has] - 6).tolist()) and {127, 128} <= set((rects["h"][has] - 6).tolist())
    assert {126, 128, 16383, 16384} <= set((rects["w"][has].astype(np.int64) * rects["h"][has]).tolist())
    assert set(FIELD_EDGES) <= set((rects["x0"][has] + 3).tolist())
    assert set(FIELD_EDGES) <= set((rects["y0"][has] + rects["h"][has].astype(np.int64) - 27).tolist())
    assert int((~has).sum()) == 3
    # the message lengths, read from the arena: the varint behind every entry's 0x1A tag
    msgs = set()
    for r, a, c in zip(rects, at, cases):
        start = int(a) - K.front_len(r, c[0], c[1])
        assert arena[start] == 0x1A
        v, s, i = 0, 0, start + 1
        while True:
            v |= (int(arena[i]) & 0x7F) << s
            s += 7
            i += 1
            if not arena[i - 1] & 0x80:
                break
        msgs.add(v)
    assert set(MSG_EDGES) <= msgs
    _check_arena(vg, fam, [(0, 0, 65535, 0)], rects, arena, at, begin)


def test_entries_per_task_equal_the_host_encoder(vg, dev):
    ctx, fam = dev
    few = TASKS[:3] + TASKS[4:]
    rects, arena, at, begin = _run(ctx, fam, few, expect_in_place=True)      # stored behind the plan, beside the raster
    _check_arena(vg, fam, few, rects, arena, at, begin)
    rects, arena, at, begin = _run(ctx, fam, TASKS)
    _check_arena(vg, fam, TASKS, rects, arena, at, begin, direct=False)
    assert len(rects) > 256


def test_rooms_and_bitmaps_are_those_of_the_resident_form(vg, dev):
    """the same arena filled with the same pattern: outside the entries' own bytes — the rooms, every bitmap — the two runs agree,
    and the resident form leaves what the ranges form fills in"""
    ctx, fam = dev
    tasks = TASKS[:3] + TASKS[4:]                                         # (few enough spans for the first guess of a context to hold)
    rects, arena, at, begin = _run(ctx, fam, tasks, expect_in_place=True)
    args, pbf, ids, adv, first_glyph = K.sequence([fam], tasks, True)
    ctx.outlines_submit_resident(*args, capacity=CAPACITY, fill=FILL, **pbf)
    r2, a2, ob2, _ = ctx.outlines_wait()
    assert np.array_equal(r2, rects) and ob2 == len(arena) and np.array_equal(ctx.outlines_pbf_positions(), at)
    mine = np.zeros(len(arena), bool)                                     # bytes the device's entries own
    for g, (r, a) in enumerate(zip(rects, at)):
        px = int(r["w"]) * int(r["h"]) if r["has_raster"] else 0
        front = K.front_len(r, int(ids[g]), int(adv[g]))
        nxt = int(at[g + 1]) - K.front_len(rects[g + 1], int(ids[g + 1]), int(adv[g + 1])) - int(pbf["pbf_pre"][g + 1]) if g + 1 < len(at) else len(arena)
        mine[int(a) - front:int(a)] = True
        mine[int(a) + px:nxt] = True
    assert np.array_equal(arena[~mine], a2[~mine]) and (a2[mine] == FILL).all() and int((~mine).sum()) > 0
    assert not (arena[mine] == FILL).all()


def test_a_pageable_output_buffer(vg, dev):
    ctx, fam = dev
    rects, arena, at, begin = _run(ctx, fam, TASKS, pinned=False)
    _check_arena(vg, fam, TASKS, rects, arena, at, begin, direct=False)


def test_a_guess_that_does_not_hold_still_delivers_the_entries(vg, dev):
    """a one-glyph submission first: the raster grid guessed from it is too small for the next batch, PlanHeader::ok stays 0,
    nothing is stored behind the plan and vgsdf_outlines_wait launches raster and entries again; then an arena that does not
    fit at all (vgsdf_outlines_render delivers it)"""
    ctx, fam = dev
    one = [(0, 200, 200, 4)]
    rects, arena, at, begin = _run(ctx, fam, one)
    _check_arena(vg, fam, one, rects, arena, at, begin)
    rects, arena, at, begin = _run(ctx, fam, TASKS, expect_in_place=False)
    _check_arena(vg, fam, TASKS, rects, arena, at, begin, direct=False)
    rects, arena, at, begin = _run(ctx, fam, TASKS, capacity=64)
    _check_arena(vg, fam, TASKS, rects, arena, at, begin, direct=False)
