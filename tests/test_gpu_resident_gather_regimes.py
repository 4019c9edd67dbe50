"""The upload kernel of submissions against command fonts (resident_gather, csrc/input_form_kernels.hip) at its edges: 256 glyphs
per workgroup, the bisection over offsets that glyphs without commands share, a glyph of more commands than a workgroup deals
in a round, records that are 4-byte aligned only, context bytes at every pair of byte offsets in store and batch, the 128 font
references a workgroup keeps in LDS, both block layouts, and the context-pass route of batches with an odd scale.

The fonts are synthetic: command records made in numpy, no font file.  The yardstick is the packed form of the same glyph
sequence (vgsdf_outlines_submit_packed): rects, sizes, every segment bit for bit, every bitmap, the positions and bitmaps of
the in-place PBF arena — tests/test_gpu_resident_fonts.py's comparison, imported.  No tolerance appears anywhere.
"""
import itertools

import numpy as np
import pytest

from test_gpu_resident_fonts import _assert_same

pytestmark = pytest.mark.gpu

GROUP = 256          # glyphs per workgroup of the upload kernel (kExpandThreads)
ROUND = 4 * GROUP    # commands a workgroup deals per round (kExpandThreads * kGatherUnroll)
FONT_CACHE = 128     # kExpandFontCache
CAPACITY = 8 << 20
E_ARG = -1
MOVE, LINE, QUAD, CURVE, CLOSE = range(5)

# glyph id -> number of commands.  0: no outline; 1 .. 7: every residue of the context bytes' offsets; 5000: more than a round
LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 12, 16, 23, 31, 40, 64, 0, 100, 257, 5000, 8, 11, 0]
BIG = LENGTHS.index(5000)
EMPTY = [i for i, n in enumerate(LENGTHS) if n == 0]
N_KINDS = 3          # fonts of one structure whose coordinates differ: a mixed-up font reference moves every outline


def _glyph(vg, n_cmds, seed, kind):
    """n_cmds command records: contours (move, lines / quads / curves in turn, close) on a grid of cells; a contour that the
    count cuts short stays open, a count of 1 is a lone move"""
    from versatiles_glyphs_rs_amd.device import OUTLINE_CMD_DTYPE
    out = np.zeros(n_cmds, dtype=OUTLINE_CMD_DTYPE)
    at, contour = 0, 0
    sx, sy, dy = ((1.0, 1.0, 0.0), (0.5, 0.75, 300.0), (1.0, -1.0, 900.0))[kind]
    while at < n_cmds:
        m = min(n_cmds - at, 5 + (seed + contour) % 6)
        cx, cy = 90.0 + 60.0 * (contour % 14), 90.0 + 60.0 * ((contour // 14) % 14)
        corners = max(m - 2, 1) + 1
        for k in range(m):
            c = out[at + k]
            a = 2.0 * np.pi * min(k, corners - 1) / corners + 0.1 * seed
            x, y = cx + 27.0 * np.cos(a), cy + 27.0 * np.sin(a)
            b = a - np.pi / corners
            c["x"], c["y"] = sx * x, sy * y + dy
            if k == 0:
                c["kind"] = MOVE
            elif k == m - 1 and m > 2:
                c["kind"] = CLOSE
                c["x"] = c["y"] = 0.0
            else:
                c["kind"] = (LINE, QUAD, CURVE)[(k + contour + seed) % 3]
                if c["kind"] >= QUAD:
                    c["x1"], c["y1"] = sx * (cx + 36.0 * np.cos(b)), sy * (cy + 36.0 * np.sin(b)) + dy
                if c["kind"] == CURVE:
                    c["x2"], c["y2"] = sx * (cx + 33.0 * np.cos(a - 0.2)), sy * (cy + 33.0 * np.sin(a - 0.2)) + dy
        at += m
        contour += 1
    return out


@pytest.fixture(scope="module")
def faces(vg):
    """-> N_KINDS descriptions (cmd_off, dat_off, kinds, coords), one per kind of font"""
    out = []
    for kind in range(N_KINDS):
        glyphs = [_glyph(vg, n, gid, kind) for gid, n in enumerate(LENGTHS)]
        cmd_off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.uint32)
        dat_off, kinds, coords = vg.SdfContext.pack_outlines(cmd_off, np.concatenate(glyphs))
        out.append((cmd_off, dat_off, kinds, coords))
    assert set(np.unique(out[0][2])) == {MOVE, LINE, QUAD, CURVE, CLOSE}
    return out


def _packed(faces, font_list, font_of, gid):
    """the packed form of the glyph sequence: glyph i is glyph id gid[i] of the font font_list[font_of[i]]"""
    cmd_off, dat_off, kinds, coords = [0], [0], [], []
    for fo, g in zip(font_of, gid):
        co, do, kk, cc = faces[font_list[fo]]
        kinds.append(kk[co[g]:co[g + 1]])
        coords.append(cc[do[g]:do[g + 1]])
        cmd_off.append(cmd_off[-1] + len(kinds[-1]))
        dat_off.append(dat_off[-1] + len(coords[-1]))
    return (np.array(cmd_off, np.uint32), np.array(dat_off, np.uint32), np.concatenate(kinds) if kinds else np.zeros(0, np.uint8),
            np.concatenate(coords) if coords else np.zeros(0, np.float32))


def _pbf(n):
    """in-place PBF arrays for n glyphs: room for a block header in front of every 100th, two- and three-byte fields"""
    pre = np.zeros(n, np.uint32)
    pre[::100] = 23
    fix = np.full(n, 2 | (3 << 4), np.uint8)
    fix[1::3] = 3 | (2 << 4)
    return dict(pbf_pre=pre, pbf_fix=fix)


def _scales(n):
    return (24.0 / 1000.0) * np.array([1.0, 0.5, 0.75])[np.arange(n) % 3], ((np.arange(n) * 37) % 100) / 100.0 - 0.5


def _compare(ctx, faces, handles, font_list, font_of, gid, scale=None, shift=None, layouts=(False, True)):
    """one glyph sequence by name against command fonts and in the packed form, with and without the PBF arrays -> the rects"""
    font_of, gid = np.asarray(font_of, np.int64), np.asarray(gid, np.int64)
    n = len(gid)
    s0, h0 = _scales(n)
    scale, shift = s0 if scale is None else scale, h0 if shift is None else shift
    form = _packed(faces, font_list, font_of, gid)
    fonts = [handles[k] for k in font_list]
    for with_pbf in layouts:
        pbf = _pbf(n) if with_pbf else {}
        ctx.outlines_submit_packed(*form, scale, shift, capacity=CAPACITY, **pbf)
        want = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf else None)
        ctx.outlines_submit_resident(fonts, font_of, gid, scale, shift, capacity=CAPACITY, **pbf)
        got = ctx.outlines_wait(), ctx.outlines_segments(), (ctx.outlines_pbf_positions() if pbf else None)
        _assert_same(got, want)
        assert ctx.resident_upload_bytes() == -(-(20 * n + 4 + 4 * n + (5 * n if with_pbf else 0)) // 16) * 16 + 32 * len(fonts)
    rects = want[0][0]
    lengths = np.array(LENGTHS)[gid]
    assert (rects["n_segments"][lengths == 0] == 0).all() and (rects["has_raster"][lengths == 0] == 0).all()
    if np.all(np.isfinite(scale)):     # a first contour of four commands or more is a polygon with an area
        assert (rects["n_segments"][lengths >= 4] > 0).all()
    return rects


@pytest.fixture()
def dev(vg, faces):
    ctx = vg.SdfContext(0)
    handles = [ctx.font_create_commands(*f) for f in faces]
    try:
        yield ctx, handles
    finally:
        ctx.close()


def test_the_restated_constants_are_the_kernels(vg):
    import ctypes as C
    cache = C.c_uint32()
    vg.load_library().vgsdf_glyf_limits(None, None, C.byref(cache))
    assert cache.value == FONT_CACHE


def test_a_store_holds_29_bytes_per_command_and_4_per_glyph_id(dev, faces):
    _, handles = dev
    n_cmds, n_ids = int(faces[0][0][-1]), len(LENGTHS)
    assert all(29 * n_cmds + 4 * (n_ids + 1) <= h.device_bytes <= (29 * n_cmds + 4 * (n_ids + 1)) * 5 // 4 + 512 for h in handles)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_glyph_counts_around_the_workgroup_size(dev, faces, n):
    ctx, handles = dev
    rng = np.random.default_rng(n)
    small = [i for i, ln in enumerate(LENGTHS) if ln <= 100]
    gid = rng.choice(small, n)
    gid[0] = LENGTHS.index(40)
    rects = _compare(ctx, faces, handles, [0], np.zeros(n, int), gid)
    assert int(rects["has_raster"].sum()) >= 1


EMPTY_POSITIONS = {
    "first": (40, [0]),
    "last": (40, [39]),
    "alone": (1, [0]),
    "runs_of_1_and_2": (60, [7, 20, 21]),
    "a_run_of_300": (700, list(range(150, 450))),
    "a_run_across_the_boundary": (600, list(range(GROUP - 6, GROUP + 7))),
    "first_and_last_of_a_workgroup": (600, [0, GROUP - 1, GROUP, 2 * GROUP - 1, 2 * GROUP, 599]),
    "a_whole_workgroup": (3 * GROUP + 10, list(range(GROUP, 2 * GROUP))),
    "the_whole_submission": (300, list(range(300))),
}


@pytest.mark.parametrize("where", list(EMPTY_POSITIONS))
def test_glyphs_without_commands(dev, faces, where):
    ctx, handles = dev
    n, empty_at = EMPTY_POSITIONS[where]
    rng = np.random.default_rng(len(where))
    full = [i for i, ln in enumerate(LENGTHS) if 4 <= ln <= 64]
    gid = rng.choice(full, n)
    gid[empty_at] = rng.choice(EMPTY, len(empty_at))
    rects = _compare(ctx, faces, handles, [1], np.zeros(n, int), gid)
    assert (rects["has_raster"][empty_at] == 0).all() and (rects["n_segments"][empty_at] == 0).all()
    assert int((rects["n_segments"] > 0).sum()) == n - len(empty_at)


def test_a_glyph_of_more_commands_than_a_round(dev, faces):
    ctx, handles = dev
    assert LENGTHS[BIG] > ROUND and LENGTHS[BIG] % ROUND not in (0, GROUP)
    small = [3, 5, 9, 13, 0, 7]
    for gid in ([BIG], small + [BIG] + small, [BIG, BIG], [BIG] + small, small + [BIG],
                # as the last glyph of a workgroup and as the first of the next
                [5] * (GROUP - 1) + [BIG, BIG] + [9] * 10):
        _compare(ctx, faces, handles, [2], np.zeros(len(gid), int), gid)


def test_context_bytes_at_every_pair_of_byte_offsets(dev, faces):
    """lengths 1 .. 7 in every order of a set of permutations: the store offset of a glyph's context bytes is fixed by its id,
    the batch offset by what stands in front of it — all 16 pairs of residues mod 4 occur (asserted)"""
    ctx, handles = dev
    ids = [LENGTHS.index(n) for n in range(1, 8)]
    perms = list(itertools.permutations(ids))[::97]
    store_off = faces[0][0].astype(np.int64)
    pairs = set()
    for perm in perms:
        at = 0
        for g in perm:
            pairs.add((int(store_off[g]) % 4, at % 4))
            at += LENGTHS[g]
    assert len(pairs) == 16
    gid = np.array([g for perm in perms for g in perm])
    assert len(gid) > GROUP
    _compare(ctx, faces, handles, [0], np.zeros(len(gid), int), gid)
    for perm in perms[:6]:
        _compare(ctx, faces, handles, [0], np.zeros(7, int), perm, layouts=(False,))


def test_repeated_ids_and_descending_order(dev, faces):
    ctx, handles = dev
    ids = np.arange(len(LENGTHS))
    _compare(ctx, faces, handles, [0], np.zeros(len(ids), int), ids[::-1])
    gid = np.array([12, 12, 12, 7, 7, BIG, 12, 0, 0, 7] * 30)
    _compare(ctx, faces, handles, [1], np.zeros(len(gid), int), gid)


@pytest.mark.parametrize("n_fonts", [1, 128, 129, 130])
def test_font_lists_around_the_cache_size(dev, faces, n_fonts):
    """the same three handles listed again and again: entry i is kind i % 3, so the entries around the cache's end (127 | 128)
    and the list's ends are fonts whose outlines differ"""
    ctx, handles = dev
    font_list = [i % N_KINDS for i in range(n_fonts)]
    wanted = [i for i in (0, 1, 126, 127, 128, 129) if i < n_fonts]
    assert len({font_list[i] for i in wanted}) >= min(n_fonts, 2)
    rng = np.random.default_rng(n_fonts)
    usable = [i for i, ln in enumerate(LENGTHS) if ln <= 100]
    # cached and uncached indices side by side in every workgroup
    n = 2 * GROUP + 77
    _compare(ctx, faces, handles, font_list, np.array(wanted)[np.arange(n) % len(wanted)], rng.choice(usable, n))
    # every index of the list once, and the long glyph from the list's last font
    font_of = np.concatenate([np.arange(n_fonts), [n_fonts - 1] * 2])
    _compare(ctx, faces, handles, font_list, font_of, np.concatenate([rng.choice(usable, n_fonts), [BIG, 12]]), layouts=(True,))


def test_odd_scales_take_the_context_pass(dev, faces):
    """a negative scale on a glyph with an outline, an infinite and a NaN one on glyphs without: the gathered context bytes
    lack the bit only the context pass forms, so it runs over the gathered records"""
    ctx, handles = dev
    gid = np.array([12, 13, EMPTY[0], 14, EMPTY[1], 15, BIG] * 40)
    n = len(gid)
    scale, shift = _scales(n)
    scale = scale.copy()
    scale[np.flatnonzero(gid == 13)[::2]] *= -1.0
    scale[np.flatnonzero(gid == EMPTY[0])[0]] = np.inf
    scale[np.flatnonzero(gid == EMPTY[1])[-1]] = np.nan
    assert (scale < 0).sum() >= 10 and np.isinf(scale).sum() == 1 and np.isnan(scale).sum() == 1 and n > GROUP
    _compare(ctx, faces, handles, [0], np.zeros(n, int), gid, scale=scale, shift=shift)
    for odd in (-0.02, np.inf, np.nan):   # one at a time
        s = _scales(5)[0].copy()
        s[2] = odd
        _compare(ctx, faces, handles, [2], np.zeros(5, int), [12, 13, EMPTY[0] if odd != -0.02 else 14, 15, 9], scale=s, shift=np.zeros(5),
                 layouts=(False,))


def test_bad_descriptions_are_refused_and_the_context_goes_on(vg, dev, faces):
    import ctypes as C
    from versatiles_glyphs_rs_amd.device import _CFontCmdsDesc
    ctx, handles = dev
    cmd_off, dat_off, kinds, coords = faces[0]

    def refused(**change):
        args = dict(cmd_off=cmd_off, dat_off=dat_off, kinds=kinds, coords=coords)
        args.update(change)
        with pytest.raises(vg.VgsdfError) as e:
            ctx.font_create_commands(**args)
        assert e.value.code == E_ARG
        gid = [12, 5, 0, BIG, 7]
        _compare(ctx, faces, handles, [0], np.zeros(len(gid), int), gid, layouts=(False,))   # the context renders the next batch

    bad = cmd_off.copy()
    bad[5], bad[6] = bad[6], bad[5]                        # not ascending
    refused(cmd_off=bad)
    bad = dat_off.copy()
    bad[10], bad[11] = bad[11], bad[10]
    refused(dat_off=bad)
    bad = cmd_off.copy()
    bad[-1] += 1                                           # does not end at n_cmds
    refused(cmd_off=bad)
    bad = kinds.copy()
    bad[int(cmd_off[12]) + 1] = 5                          # a kind of 5
    refused(kinds=bad)
    for delta in (-1, 1):                                  # a glyph whose dat_off range is one float short / long
        bad = dat_off.astype(np.int64)
        bad[13:] += delta
        refused(dat_off=bad, coords=np.concatenate([coords, [0.0]]) if delta > 0 else coords[:-1])
    bad = dat_off.copy()                                   # ... with the face's total unchanged (the next glyph makes up for it)
    bad[13] -= 1
    refused(dat_off=bad)
    # a store past what 32-bit offsets address (29 bytes per command): refused before anything is read or allocated
    huge = 150_000_000
    refused(cmd_off=np.array([0, huge], np.uint32), dat_off=np.zeros(2, np.uint32), kinds=np.zeros(huge, np.uint8), coords=np.zeros(0, np.float32))
    # NULL arrays
    L = vg.load_library()
    p = lambda a: a.ctypes.data  # noqa: E731
    for null in ("cmd_off", "dat_off", "kinds", "coords"):
        d = _CFontCmdsDesc(len(cmd_off) - 1, len(kinds), len(coords), p(cmd_off), p(dat_off), p(kinds), p(coords))
        setattr(d, null, None)
        h = C.c_void_p()
        assert L.vgsdf_font_create_commands(ctx._h, C.byref(d), C.byref(h)) == E_ARG and not h.value
    h = C.c_void_p()
    assert L.vgsdf_font_create_commands(ctx._h, None, C.byref(h)) == E_ARG
    _compare(ctx, faces, handles, [0], np.zeros(3, int), [12, 13, 14], layouts=(False,))
    # a face without a single command is a face of glyphs without outline
    none = ctx.font_create_commands(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.float32))
    ctx.outlines_submit_resident([none], [0, 0], [2, 0], [0.024, 0.024], [0.0, 0.0], capacity=1 << 16)
    rects = ctx.outlines_wait()[0]
    assert (rects["has_raster"] == 0).all() and (rects["n_segments"] == 0).all()


def test_bad_submissions_are_refused_and_the_context_goes_on(vg, dev, faces):
    from test_gpu_resident_fonts import _font_set
    ctx, handles = dev
    _, _, _, _, descs = _font_set(vg, "fira")
    glyf_font = ctx.font_create(descs[0]["leaf_off"], descs[0]["leaves"], descs[0]["bytes"])
    scale, shift = _scales(4)

    def refused(fonts, font_of, gid):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.outlines_submit_resident(fonts, font_of, gid, scale, shift, capacity=1 << 20)
        assert e.value.code == E_ARG
        _compare(ctx, faces, handles, [1], np.zeros(4, int), [12, 0, BIG, 7], layouts=(True,))

    refused([handles[0], glyf_font], [0, 0, 1, 0], [12, 13, 14, 15])      # fonts of both kinds (named or not)
    refused([glyf_font, handles[0]], [0, 0, 0, 0], [12, 13, 14, 15])
    refused([handles[0]], [0, 0, 0, 0], [12, len(LENGTHS), 14, 15])       # a glyph id past the face
    refused([handles[0]], [0, 1, 0, 0], [12, 13, 14, 15])                 # font_of past n_fonts
    # either kind alone still renders on this context
    ctx.outlines_submit_resident([glyf_font], [0, 0, 0, 0], [40, 41, 42, 43], scale, shift, capacity=1 << 20)
    assert int(ctx.outlines_wait()[0]["has_raster"].sum()) >= 1


def test_a_command_font_is_shared_by_the_contexts_of_its_device(vg, dev, faces):
    a, handles = dev
    b = vg.SdfContext(0)
    try:
        gid = np.array([12, 13, BIG, 0, 14, 15] * 50)
        n = len(gid)
        scale, shift = _scales(n)
        form = _packed(faces, [0], np.zeros(n, int), gid)
        a.outlines_submit_packed(*form, scale, shift, capacity=CAPACITY)
        want = a.outlines_wait()
        half = n // 2
        # created through one context, named by two, both in flight at once
        a.outlines_submit_resident([handles[0]], np.zeros(half, int), gid[:half], scale[:half], shift[:half], capacity=CAPACITY)
        b.outlines_submit_resident([handles[0]], np.zeros(n - half, int), gid[half:], scale[half:], shift[half:], capacity=CAPACITY)
        ra, rb = a.outlines_wait(), b.outlines_wait()
        assert np.array_equal(np.concatenate([ra[0], rb[0]]), want[0])
        assert np.array_equal(np.concatenate([ra[1], rb[1]]), want[1])
    finally:
        b.close()
