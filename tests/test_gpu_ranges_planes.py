"""One ranges submission over families of DIFFERENT planes (vgsdf_outlines_submit_ranges; csrc/family_upload_kernel.inc with the
family's cp_base): the plane-0 and the plane-1 family of Noto Sans Regular, both built on the device from its cmap and hmtx
(vgsdf_family_create_tables_at), named alternately by tasks that include the whole plane (first 0x0000, last 0xFFFF), single
blocks, U+1DF00's block — whose LOW halves lie in D800 .. DFFF —, tasks that map nothing and tasks that repeat; with pbf_pre NULL
and given, over glyf and over command stores.  The yardstick is vgsdf_outlines_submit_resident of the same glyph sequence with
pbf_fix from the FULL ids, as include/vgsdf.h states it: rects, sizes, every segment bit for bit, every bitmap, every position;
and the entries the device wrote are vg_pbf_encode's of the rects and bitmaps read back, with the full code points as ids — 3-byte
varints in plane 1, 1 to 3 bytes in plane 0.  No tolerance appears anywhere."""
import numpy as np
import pytest

import family_ranges_kit as K
from conftest import noto_files
from test_gpu_pbf_entries_device import _expected_entries
from test_gpu_resident_fonts import _assert_same

pytestmark = pytest.mark.gpu

CAPACITY = 16 << 20
# (family = plane, first, last, pbf_pre) on low halves
TASKS = [(0, 0x0000, 0xFFFF, 21), (1, 0x0000, 0xFFFF, 9), (0, 0x0041, 0x005A, 5), (1, 0x0700, 0x07FF, 7), (0, 0xD800, 0xDFFF, 3),
         (1, 0x0000, 0x06FF, 4), (0, 0x0041, 0x005A, 5), (1, 0x0700, 0x07FF, 7), (1, 0xDF00, 0xDFFF, 0), (0, 0x0000, 0x007F, 0),
         (1, 0xE000, 0xFFFF, 2)]


@pytest.fixture(scope="module", params=["glyf", "commands"])
def dev(vg, request):
    path = next(p for p in noto_files() if p.stem == "Noto Sans - Regular")
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name("Noto Sans Regular", [path])
    desc = mgr.family_tables_desc(fid, 0)
    ctx = vg.SdfContext(0)
    try:
        if request.param == "glyf":
            d = mgr.resident_font_desc(fid, 0)
            font = ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"])
        else:
            d = mgr.command_font_desc(fid, 0)
            font = ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"])
        fams = [ctx.family_create_tables_at([font], [desc], plane) for plane in (0, 1)]
        yield ctx, font, fams, [ctx.family_read(f) for f in fams]
        for f in fams:
            f.free()
    finally:
        ctx.close()


def sequence(font, tables, tasks, with_pre):
    """the arguments of outlines_submit_resident for the glyphs the tasks stand for, their FULL ids, advances and per task its glyphs"""
    font_of, gid, scale, shift, pre, ids, adv, counts = [], [], [], [], [], [], [], []
    for k, a, b, room in tasks:
        t = tables[k]
        e = np.flatnonzero((t["code_point"] >= a) & (t["code_point"] <= b))
        counts.append(len(e))
        font_of.append(np.full(len(e), k)), gid.append(t["glyph_id"][e]), scale.append(t["scale"][e]), shift.append(t["shift_x"][e])
        ids.append(t["code_point"][e].astype(np.uint32) + (k << 16)), adv.append(t["advance"][e])
        p = np.zeros(len(e), np.uint32)
        p[:1] = room
        pre.append(p)
    ids, adv = np.concatenate(ids).astype(np.uint32), np.concatenate(adv).astype(np.uint32)
    pbf = dict(pbf_pre=np.concatenate(pre), pbf_fix=K.fix_of(ids, adv)) if with_pre else {}
    args = ([font, font], np.concatenate(font_of).astype(np.uint16), np.concatenate(gid).astype(np.uint16), np.concatenate(scale), np.concatenate(shift))
    return args, pbf, ids, adv, counts


def test_the_two_planes_of_noto_sans_regular(dev):
    ctx, font, fams, tables = dev
    assert [f.plane for f in fams] == [0, 1]
    assert len(tables[0]["code_point"]) + len(tables[1]["code_point"]) == 3094 and len(tables[1]["code_point"]) == 88
    low = tables[1]["code_point"]
    assert set((low >> 8).tolist()) == {0x07, 0xDF} and ((tables[1]["pbf_fix"] & 15) == 4).all()
    assert set((tables[0]["pbf_fix"] & 15).tolist()) == {2, 3, 4}            # ids of 1, 2 and 3 bytes
    assert fams[1].count(0xD800, 0xDFFF) == int((low >= 0xDF00).sum()) > 0 and fams[0].count(0xD800, 0xDFFF) == 0


@pytest.mark.parametrize("with_pre", [False, True], ids=["packed_bitmaps", "pbf_pre"])
def test_alternating_planes_equal_the_resident_form_with_full_ids(vg, dev, with_pre):
    ctx, font, fams, tables = dev
    fam_of, first, last, room = [np.array([t[i] for t in TASKS], np.int64) for i in range(4)]
    args, pbf, ids, adv, counts = sequence(font, tables, TASKS, with_pre)
    n = len(ids)
    assert counts[4] == 0 and counts[5] == 0 and counts[10] == 0 and counts[0] == 3006 and counts[1] == 88 and counts[2] == counts[6] == 26
    assert counts[3] == counts[7] > 0 and counts[8] > 0 and counts[3] + counts[8] == 88
    ctx.outlines_submit_resident(*args, capacity=CAPACITY, **pbf)
    want = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if with_pre else None)
    ctx.outlines_submit_ranges(fams, fam_of, first, last, capacity=CAPACITY, pbf_pre=room if with_pre else None)
    got = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if with_pre else None)
    _assert_same(got, want)
    rects, arena = got[0][0], got[0][1]
    assert len(rects) == n == sum(counts) and ctx.resident_upload_bytes() == 32 * (sum(1 for c in counts if c) + 2 + 2)
    if not with_pre:
        return
    at, begin = got[2], ctx.outlines_task_extents()
    assert len(begin) == len(TASKS) + 1 and int(begin[0]) == 0 and int(begin[-1]) == len(arena) == got[0][2]
    g = 0
    for t, c in enumerate(counts):
        lo, hi = int(begin[t]), int(begin[t + 1])
        if c == 0:
            assert lo == hi
            continue
        plane = TASKS[t][0]
        assert (ids[g:g + c] >> 16 == plane).all()
        entries = _expected_entries(vg, rects[g:g + c], arena, at[g:g + c], ids[g:g + c], adv[g:g + c])
        assert arena[lo + int(room[t]):hi].tobytes() == entries.tobytes(), f"task {t}"
        # the id the device wrote in front of the first glyph's bitmap: 0x08 and the varint of the FULL code point
        front = K.front_len(rects[g], int(ids[g]), int(adv[g]))
        start = lo + int(room[t])
        assert int(at[g]) - front == start and arena[start] == 0x1A
        id_len = K.varint_len(int(ids[g]))
        assert id_len == (3 if plane else K.varint_len(int(ids[g]) & 0xFFFF))
        i = start + 1
        while arena[i] & 0x80:
            i += 1
        assert arena[i + 1] == 0x08
        v = sum((int(arena[i + 2 + j]) & 0x7F) << (7 * j) for j in range(id_len))
        assert v == int(ids[g]) and not arena[i + 2 + id_len - 1] & 0x80
        g += c
    assert g == n
