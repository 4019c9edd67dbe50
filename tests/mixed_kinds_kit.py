"""What the tests of submissions over fonts of BOTH kinds share (no test in here): the synthetic command fonts and glyf fonts of
family_ranges_kit on ONE context, the yardstick of a mixed glyph sequence — its glyf and its command subsequence, each submitted
by the existing vgsdf_outlines_submit_resident, interleaved back into the sequence's order — and a restatement in Python of the
in-place PBF arena as include/vgsdf.h states it (vgsdf_outlines_packed).  Comparisons go through
tests/test_gpu_resident_fonts.py's _assert_same: rects, sizes, every segment bit for bit, every bitmap, every position.  No
tolerance appears anywhere."""
import numpy as np

import family_ranges_kit as K
from family_ranges_kit import varint_len
from test_gpu_resident_fonts import _assert_same

GROUP = K.GROUP              # glyphs per workgroup of the upload kernels (kExpandThreads)
ROUND = 4 * GROUP            # commands a workgroup gathers per round (kExpandThreads * kGatherUnroll)
FONT_CACHE = K.FONT_CACHE    # kExpandFontCache
CAPACITY = K.CAPACITY
E_ARG = K.E_ARG
GLYF, COMMANDS = 0, 1


class MixedKit:
    """both kits of family_ranges_kit on one context.  A font is named (kind, k): font k of the glyf kit (kind GLYF) or of the
    command kit (kind COMMANDS); small / empty / big: per kind, as family_ranges_kit.Kit has them"""

    def __init__(self, vg, ctx):
        import test_gpu_resident_expand_regimes as X
        import test_gpu_resident_gather_regimes as G
        self.ctx = ctx
        self.kits = (K.glyf_kit(vg, ctx), K.command_kit(vg, ctx))
        self.small = tuple(k.small for k in self.kits)
        self.empty = tuple(k.empty for k in self.kits)
        self.big = tuple(k.big for k in self.kits)
        self.n_kinds = tuple(len(k.kinds) for k in self.kits)
        self.n_ids = (len(X.LEAVES_PER_GLYPH), len(G.LENGTHS))
        self.command_lengths = np.array(G.LENGTHS)
        assert X.LEAVES_PER_GLYPH[self.big[GLYF]] == 600 and G.LENGTHS[self.big[COMMANDS]] == 5000

    def handle(self, font):
        kind, k = font
        return self.kits[kind].kinds[k]

    def handles(self, font_list):
        return [self.handle(f) for f in font_list]

    def slots(self, kind, gid):
        """command slots glyph id gid of a font of `kind` takes in a submission (the same for every font of a kit)"""
        if kind == COMMANDS:
            return int(self.command_lengths[gid])
        if not hasattr(self, "_glyf_slots"):
            font = self.ctx.font_read(self.kits[GLYF].kinds[0])
            ends = np.concatenate([[0], np.cumsum(font["leaves"]["cmd_cap"].astype(np.int64))])
            self._glyf_slots = np.diff(ends[font["leaf_off"].astype(np.int64)])
        return int(self._glyf_slots[gid])


def pbf_arrays(n):
    """in-place PBF arrays for n glyphs: room for a block header in front of every 100th, two- and three-byte fields"""
    pre = np.zeros(n, np.uint32)
    pre[::100] = 23
    fix = np.full(n, 2 | (3 << 4), np.uint8)
    fix[1::3] = 3 | (2 << 4)
    return dict(pbf_pre=pre, pbf_fix=fix)


def scales(n):
    return (24.0 / 1000.0) * np.array([1.0, 0.5, 0.75])[np.arange(n) % 3], ((np.arange(n) * 37) % 100) / 100.0 - 0.5


def arena(rects, pbf_pre, pbf_fix):
    """include/vgsdf.h, vgsdf_outlines_packed: glyph g starts at the running sum of what the glyphs before it occupy plus
    pbf_pre[g]; its entry is 0x1A varint(len) | 0x08 varint(id) | [0x12 varint(w h) BITMAP] | 0x18 width 0x20 height 0x28 left
    0x30 top 0x38 advance with width = w - 6, height = h - 6, left = x0 + 3, top = y0 + h - 27 (sint32: zigzag), a glyph without
    a raster PbfGlyph::empty (the four fields 0, no bitmap); pbf_fix[g] = (1 + varint_len(id)) | (1 + varint_len(advance)) << 4
    -> (the position of every glyph's bitmap, the arena's size)"""
    zz = lambda v: ((v << 1) ^ (v >> 31)) & 0xFFFFFFFF  # noqa: E731
    at, run = np.zeros(len(rects), np.uint64), 0
    for g, (r, pre, fix) in enumerate(zip(rects, pbf_pre, pbf_fix)):
        id_len, adv_len = int(fix) & 15, int(fix) >> 4
        w, h, x0, y0 = int(r["w"]), int(r["h"]), int(r["x0"]), int(r["y0"])
        if r["has_raster"]:
            px = w * h
            bm_hdr = 1 + varint_len(px)
            fields = [w - 6, h - 6, zz(x0 + 3), zz(y0 + h - 27)]
        else:
            px, bm_hdr, fields = 0, 0, [0, 0, 0, 0]
        msg = id_len + bm_hdr + px + sum(1 + varint_len(v) for v in fields) + adv_len
        front = 1 + varint_len(msg) + id_len + bm_hdr
        run += int(pre)
        at[g] = run + front
        run += 1 + varint_len(msg) + msg
    return at, run


def run_resident(ctx, fonts, font_of, gid, scale, shift, mixed=False, **pbf):
    """one submission by name -> ((rects, bitmaps, out_bytes, n_segments), (seg_off, segs), positions or None)"""
    submit = ctx.outlines_submit_resident_mixed if mixed else ctx.outlines_submit_resident
    submit(fonts, np.asarray(font_of, np.int64), np.asarray(gid, np.int64), scale, shift, capacity=CAPACITY, **pbf)
    return ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf and len(gid) else None)


def yardstick(kit, font_list, font_of, gid, scale, shift, pbf):
    """the sequence's glyf and command subsequences, each by the existing call (bitmaps packed back to back), interleaved back
    -> what one submission of the whole sequence must give, in _assert_same's shape; with `pbf` the arena by the restatement,
    which is first held against the device's positions of each single-kind subsequence"""
    ctx = kit.ctx
    font_of, gid = np.asarray(font_of, np.int64), np.asarray(gid, np.int64)
    n = len(gid)
    kind_of_font = np.array([k for k, _ in font_list], np.int64)
    kind = kind_of_font[font_of] if n else np.zeros(0, np.int64)
    from versatiles_glyphs_rs_amd.device import RECT_DTYPE
    rects = np.zeros(n, RECT_DTYPE)
    segs, bitmaps = [None] * n, [None] * n
    for which in (GLYF, COMMANDS):
        at = np.flatnonzero(kind == which)
        if not len(at):
            continue
        sub_list = [i for i, (k, _) in enumerate(font_list) if k == which]      # the fonts of this kind, renumbered
        renumber = {f: i for i, f in enumerate(sub_list)}
        sub_font_of = np.array([renumber[f] for f in font_of[at]], np.int64)
        fonts = kit.handles([font_list[i] for i in sub_list])
        (r, bm, _, _), (so, sg), _ = run_resident(ctx, fonts, sub_font_of, gid[at], scale[at], shift[at])
        assert bm is not None
        rects[at] = r
        px = np.where(r["has_raster"] != 0, r["w"].astype(np.int64) * r["h"].astype(np.int64), 0)
        bo = np.concatenate([[0], np.cumsum(px)])
        assert bo[-1] == len(bm)
        for j, g in enumerate(at):
            segs[g] = sg[int(so[j]):int(so[j + 1])]
            bitmaps[g] = bm[int(bo[j]):int(bo[j + 1])]
        if pbf:   # the restatement reproduces the positions of a submission of ONE kind before it is used on the sequence
            sub = dict(pbf_pre=pbf["pbf_pre"][at], pbf_fix=pbf["pbf_fix"][at])
            (r2, _, ob2, _), _, at2 = run_resident(ctx, fonts, sub_font_of, gid[at], scale[at], shift[at], **sub)
            want_at, want_size = arena(r2, sub["pbf_pre"], sub["pbf_fix"])
            assert np.array_equal(r2, r) and np.array_equal(at2, want_at) and ob2 == want_size
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint32)
    all_segs = np.concatenate(segs) if n and int(seg_off[-1]) else np.zeros((0, 4))
    if pbf:
        at, size = arena(rects, pbf["pbf_pre"], pbf["pbf_fix"])
        out = np.zeros(size, np.uint8)
        for g in range(n):
            out[int(at[g]):int(at[g]) + len(bitmaps[g])] = bitmaps[g]
    else:
        at, out = None, (np.concatenate(bitmaps) if n else np.zeros(0, np.uint8))
    return (rects, out, len(out), int(seg_off[-1])), (seg_off, all_segs), at


def upload_bytes(n, n_fonts, with_pbf):
    """the block of a mixed submission: the glyf form's (33 n + 8 with the PBF arrays), 16-aligned, and 32 bytes per font"""
    return -(-(16 * n + 4 * (n + 1) + 4 * (n + 1) + 4 * n + (5 * n if with_pbf else 0)) // 16) * 16 + 32 * n_fonts


def compare(kit, font_list, font_of, gid, scale=None, shift=None, layouts=(False, True)):
    """one mixed submission against the yardstick, without and with the PBF arrays -> the rects"""
    font_of, gid = np.asarray(font_of, np.int64), np.asarray(gid, np.int64)
    n = len(gid)
    s0, h0 = scales(n)
    scale, shift = s0 if scale is None else np.asarray(scale, np.float64), h0 if shift is None else np.asarray(shift, np.float64)
    fonts = kit.handles(font_list)
    rects = None
    for with_pbf in layouts:
        pbf = pbf_arrays(n) if with_pbf else {}
        want = yardstick(kit, font_list, font_of, gid, scale, shift, pbf)
        got = run_resident(kit.ctx, fonts, font_of, gid, scale, shift, mixed=True, **pbf)
        _assert_same(got, want)
        assert kit.ctx.resident_upload_bytes() == upload_bytes(n, len(fonts), with_pbf)
        rects = want[0][0]
    return rects


def glyphs(kit, rng, kinds, fonts=None):
    """kinds: per glyph GLYF or COMMANDS -> (font_list, font_of, gid) over the first font of either kit (or `fonts`, one per
    kind), glyph ids with a small outline"""
    fonts = fonts or ((GLYF, 0), (COMMANDS, 0))
    kinds = np.asarray(kinds, np.int64)
    gid = np.where(kinds == GLYF, rng.choice(kit.small[GLYF], len(kinds)), rng.choice(kit.small[COMMANDS], len(kinds)))
    return list(fonts), kinds.copy(), gid


# ---- mixed families ----

class MixedFamily:
    """a mixed family over `font_list` ((kind, k) pairs) and its description's arrays; sequence() of family_ranges_kit reads it
    as it reads a Family"""

    def __init__(self, kit, font_list, code_point, font_of, glyph_id, advance, scale, shift_x, create=True):
        self.kit, self.font_list = kit, list(font_list)
        self.cp, self.font_of, self.gid = np.asarray(code_point, np.int64), np.asarray(font_of, np.int64), np.asarray(glyph_id, np.int64)
        self.advance, self.scale, self.shift = np.asarray(advance, np.uint32), np.asarray(scale, np.float64), np.asarray(shift_x, np.float64)
        self.fonts = kit.handles(self.font_list)
        self.handle = kit.ctx.family_create_mixed(self.fonts, self.cp, self.font_of, self.gid, self.advance, self.scale, self.shift) if create else None


def random_mixed_family(kit, seed, n_entries, font_list=((GLYF, 0), (COMMANDS, 0)), font_of=None, big_at=(), empty_at=(), first_cp=3,
                        gaps=(1, 2, 3)):
    """n_entries code points from first_cp on; entry i belongs to font font_of[i] (default: alternating through font_list);
    glyph ids with a small outline of the font's kind but for the entries big_at (the kind's very large glyph) and empty_at
    (glyph ids without outline)"""
    rng = np.random.default_rng(seed)
    cp = first_cp + np.cumsum(rng.choice(gaps, n_entries)) - 1
    assert cp[-1] <= 0xFFFF
    font_of = np.arange(n_entries) % len(font_list) if font_of is None else np.asarray(font_of, np.int64)
    kind = np.array([k for k, _ in font_list], np.int64)[font_of]
    gid = np.where(kind == GLYF, rng.choice(kit.small[GLYF], n_entries), rng.choice(kit.small[COMMANDS], n_entries))
    for i in big_at:
        gid[i] = kit.big[kind[i]]
    for i in empty_at:
        gid[i] = rng.choice(kit.empty[kind[i]])
    scale = (24.0 / 1000.0) * np.array([1.0, 0.5, 0.75])[rng.integers(0, 3, n_entries)]
    shift = rng.integers(0, 100, n_entries) / 100.0 - 0.5
    return MixedFamily(kit, font_list, cp, font_of, gid, K.ADVANCES[rng.integers(0, len(K.ADVANCES), n_entries)], scale, shift)


def compare_ranges(ctx, families, tasks, layouts=(False, True), capacity=CAPACITY):
    """family_ranges_kit.compare for mixed families: one ranges submission against vgsdf_outlines_submit_resident_mixed of the
    glyph sequence it stands for, without and with pbf_pre; the upload's size; with pbf_pre the tasks' extents -> the rects"""
    fam_of, first, last, room = [np.array([t[i] for t in tasks], np.int64) for i in range(4)]
    handles = [f.handle for f in families]
    rects = None
    for with_pre in layouts:
        args, pbf, ids, adv, first_glyph = K.sequence(families, tasks, with_pre)
        n = len(args[1])
        ctx.outlines_submit_resident_mixed(*args, capacity=capacity, **pbf)
        want = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf and n else None)
        ctx.outlines_submit_ranges(handles, fam_of, first, last, capacity=capacity, pbf_pre=room if with_pre else None)
        got = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf and n else None)
        _assert_same(got, want)
        n_live = sum(1 for g in first_glyph if g >= 0)
        assert ctx.resident_upload_bytes() == 32 * (n_live + len(families) + len(args[0]))
        rects = want[0][0]
        if with_pre:
            begin = ctx.outlines_task_extents()
            assert len(begin) == len(tasks) + 1 and int(begin[-1]) == want[0][2] and (np.diff(begin.astype(np.int64)) >= 0).all()
            for t, g in enumerate(first_glyph):
                if g < 0:
                    assert begin[t] == begin[t + 1]
                else:
                    assert int(begin[t]) + int(room[t]) + K.front_len(rects[g], int(ids[g]), int(adv[g])) == int(want[2][g])
            if len(tasks):
                assert begin[0] == 0
    return rects
