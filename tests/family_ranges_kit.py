"""What the tests of resident families share (no test in here): synthetic fonts of both kinds, families over them, the glyph
sequence a ranges submission stands for, and the comparison of vgsdf_outlines_submit_ranges with
vgsdf_outlines_submit_resident of that sequence — rects, sizes, every segment bit for bit, bitmaps and PBF positions through
tests/test_gpu_resident_fonts.py's _assert_same.  No tolerance appears anywhere."""
import numpy as np

from test_gpu_resident_fonts import _assert_same

GROUP = 256          # glyphs per workgroup of the upload kernels (kExpandThreads)
FONT_CACHE = 128     # kExpandFontCache
CAPACITY = 8 << 20
E_ARG = -1
# every length of a varint of a u32: the advances of the synthetic families
ADVANCES = np.array([0, 127, 128, 16383, 16384, 1 << 21, 1 << 28, (1 << 32) - 1, 13, 600], np.uint32)


def varint_len(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def fix_of(ids, advances):
    """pbf_fix as include/vgsdf.h states it: (1 + varint_len(id)) | (1 + varint_len(advance)) << 4"""
    return np.array([(1 + varint_len(int(i))) | ((1 + varint_len(int(a))) << 4) for i, a in zip(ids, advances)], np.uint8)


class Kit:
    """fonts of one kind on one context: `kinds` ResidentFont handles of fonts with the same glyph ids and differing outlines,
    small: glyph ids with a small outline that has an area, empty: glyph ids without outline, big: a glyph id of very many
    commands / leaves"""

    def __init__(self, name, ctx, kinds, small, empty, big):
        self.name, self.ctx, self.kinds, self.big = name, ctx, kinds, big
        self.small, self.empty = np.flatnonzero(small), np.flatnonzero(empty)
        assert len(self.small) >= 5 and len(self.empty) >= 2


def command_kit(vg, ctx):
    import test_gpu_resident_gather_regimes as G
    glyphs = [[G._glyph(vg, n, gid, kind) for gid, n in enumerate(G.LENGTHS)] for kind in range(G.N_KINDS)]
    cmd_off = np.concatenate([[0], np.cumsum(G.LENGTHS)]).astype(np.uint32)
    kinds = []
    for g in glyphs:
        dat_off, kk, cc = vg.SdfContext.pack_outlines(cmd_off, np.concatenate(g))
        kinds.append(ctx.font_create_commands(cmd_off, dat_off, kk, cc))
    L = np.array(G.LENGTHS)
    return Kit("commands", ctx, kinds, (L >= 4) & (L <= 100), L == 0, G.BIG)    # (4 commands and more: a polygon with an area)


def glyf_kit(vg, ctx):
    import test_gpu_resident_expand_regimes as X
    descs, _ = X._synthetic(vg)
    L = np.array(X.LEAVES_PER_GLYPH)
    return Kit("glyf", ctx, [ctx.font_create(*d) for d in descs], (L >= 1) & (L <= 5), L == 0, int(np.flatnonzero(L == 600)[0]))


def make_kit(vg, ctx, kind):
    return command_kit(vg, ctx) if kind == "commands" else glyf_kit(vg, ctx)


class Family:
    """a family over `font_list` (indices into kit.kinds) and its description's arrays"""

    def __init__(self, kit, font_list, code_point, font_of, glyph_id, advance, scale, shift_x):
        self.kit, self.font_list = kit, list(font_list)
        self.cp, self.font_of, self.gid = np.asarray(code_point, np.int64), np.asarray(font_of, np.int64), np.asarray(glyph_id, np.int64)
        self.advance, self.scale, self.shift = np.asarray(advance, np.uint32), np.asarray(scale, np.float64), np.asarray(shift_x, np.float64)
        self.fonts = [kit.kinds[k] for k in self.font_list]
        self.handle = kit.ctx.family_create(self.fonts, self.cp, self.font_of, self.gid, self.advance, self.scale, self.shift)


def random_family(kit, seed, n_entries, font_list=(0,), big_at=(), empty_at=(), first_cp=3, gaps=(1, 2, 3), odd_scale=None):
    """n_entries code points from first_cp on with gaps from `gaps`; glyph ids with an outline and few commands but for the
    entries big_at (the very large glyph) and empty_at (glyph ids without outline); every font of font_list in turn"""
    rng = np.random.default_rng(seed)
    cp = first_cp + np.cumsum(rng.choice(gaps, n_entries)) - 1
    assert cp[-1] <= 0xFFFF
    gid = rng.choice(kit.small, n_entries)
    gid[list(big_at)] = kit.big
    if len(empty_at):
        gid[list(empty_at)] = rng.choice(kit.empty, len(empty_at))
    font_of = (np.arange(n_entries) * 7 + seed) % len(font_list)
    scale = (24.0 / 1000.0) * np.array([1.0, 0.5, 0.75])[rng.integers(0, 3, n_entries)]
    if odd_scale is not None:
        scale[odd_scale[0]] = odd_scale[1]
    shift = rng.integers(0, 100, n_entries) / 100.0 - 0.5
    return Family(kit, font_list, cp, font_of, gid, ADVANCES[rng.integers(0, len(ADVANCES), n_entries)], scale, shift)


def sequence(families, tasks, with_pre):
    """tasks: [(family index, first, last, pre)] -> the arguments of outlines_submit_resident for the glyph sequence the ranges
    stand for, the ids / advances of its glyphs and the index of every task's first glyph (-1: the task maps nothing)"""
    base = np.concatenate([[0], np.cumsum([len(f.font_list) for f in families])])
    fonts = [h for f in families for h in f.fonts]
    font_of, gid, scale, shift, pre, ids, adv, first_glyph = [], [], [], [], [], [], [], []
    n = 0
    for k, a, b, room in tasks:
        f = families[k]
        e = np.flatnonzero((f.cp >= a) & (f.cp <= b))
        first_glyph.append(n if len(e) else -1)
        n += len(e)
        font_of.append(base[k] + f.font_of[e]), gid.append(f.gid[e]), scale.append(f.scale[e]), shift.append(f.shift[e])
        ids.append(f.cp[e]), adv.append(f.advance[e])
        p = np.zeros(len(e), np.uint32)
        p[:1] = room
        pre.append(p)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    ids, adv = cat(ids, np.uint32), cat(adv, np.uint32)
    pbf = dict(pbf_pre=cat(pre, np.uint32), pbf_fix=fix_of(ids, adv)) if with_pre else {}
    return (fonts, cat(font_of, np.uint16), cat(gid, np.uint16), cat(scale, np.float64), cat(shift, np.float64)), pbf, ids, adv, first_glyph


def front_len(rect, glyph_id, advance):
    """bytes of a glyph's PBF entry in front of its bitmap: 0x1A varint(msg) 0x08 varint(id) [0x12 varint(w h)]"""
    has = bool(rect["has_raster"])
    w, h, x0, y0 = int(rect["w"]), int(rect["h"]), int(rect["x0"]), int(rect["y0"])
    zz = lambda v: ((v << 1) ^ (v >> 31)) & 0xFFFFFFFF  # noqa: E731
    px = w * h if has else 0
    fields = [w - 6, h - 6, zz(x0 + 3), zz(y0 + h - 27)] if has else [0, 0, 0, 0]
    bm_hdr = 1 + varint_len(px) if has else 0
    msg = 1 + varint_len(glyph_id) + bm_hdr + px + sum(1 + varint_len(v) for v in fields) + 1 + varint_len(advance)
    return 1 + varint_len(msg) + 1 + varint_len(glyph_id) + bm_hdr


def compare(ctx, families, tasks, layouts=(False, True), capacity=CAPACITY):
    """one ranges submission against the resident form of the glyph sequence it stands for, without and with pbf_pre -> the
    rects; with pbf_pre also the tasks' extents against the positions"""
    fam_of, first, last, room = [np.array([t[i] for t in tasks], np.int64) for i in range(4)]
    handles = [f.handle for f in families]
    rects = None
    for with_pre in layouts:
        args, pbf, ids, adv, first_glyph = sequence(families, tasks, with_pre)
        n = len(args[1])
        ctx.outlines_submit_resident(*args, capacity=capacity, **pbf)
        want = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf and n else None)
        ctx.outlines_submit_ranges(handles, fam_of, first, last, capacity=capacity, pbf_pre=room if with_pre else None)
        got = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf and n else None)
        _assert_same(got, want)
        # the upload holds a record per task that maps a glyph, per family and per font, and nothing per glyph
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
                    assert int(begin[t]) + int(room[t]) + front_len(rects[g], int(ids[g]), int(adv[g])) == int(want[2][g])
            if len(tasks):
                assert begin[0] == 0
    return rects
