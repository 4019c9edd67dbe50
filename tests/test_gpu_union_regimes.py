"""GPU: the union pass (rule U; csrc/outline_union_kernels.hip) against its restatement
(tests/union_outline_kit.py), bit for bit, and the raster over its pieces against the oracle over the restated pieces.

  exact     every exact set of the kit in one batch
  counts    1 / 63 / 64 / 65 / 129 glyphs with unlike neighbours (identity, rebuilt, cancelled, empty)
  sizes     63 / 64 / 65 / 255 / 256 / 257 segments (the rounds of 256 lanes, the raster's chunks), 1023 / 1024 / 1025 (the
            window in LDS: staged once, or swept), exactly the limit and one more (passed through), a coordinate that is
            not finite (passed through), zero-length segments in a glyph that is otherwise untouched (identity)
  noto      the 38 glyphs of Noto Sans Regular's first 600 code points that rule U rebuilds (U+00C5, U+00C7, U+0104 and U+0224
            among them) and every 20th glyph of Fira Sans's first 600 (identities)
Each under both segment layouts: the four arrays of an uploaded batch (vgsdf_batch_union) and the 32-byte records of the
device front-end's batch (vgsdf_outlines_union over the same outlines given as commands: every glyph of every case but the
one with a coordinate that is not finite, which no command can carry); the passes themselves over records in plain device
memory hold that state too (test_the_passes_on_records)."""
import numpy as np
import pytest

import union_outline_kit as K
from conftest import FIRA, NOTO
from test_gpu_front_end_regimes import _stream

pytestmark = pytest.mark.gpu


def _sizes():
    glyphs = [K.sized_glyph(n) for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)]
    glyphs += [K.sized_glyph(K.UNION_MAX_SEGMENTS), K.sized_glyph(K.UNION_MAX_SEGMENTS + 1)]
    bad = K.rect_set_segments("two_rects")
    bad[5, 2] = np.inf
    glyphs.append(bad)
    zl = K.polygon(9)
    glyphs.append(np.concatenate([zl[:4], [[zl[4, 0], zl[4, 1], zl[4, 0], zl[4, 1]]], zl[4:]]))
    return glyphs


def _noto():
    noto = [segs for cp, _, segs in K.font_glyphs(NOTO, 600) if cp in K.REBUILT_NOTO]
    assert len(noto) == len(K.REBUILT_NOTO) == 38
    return noto + [segs for _, _, segs in K.font_glyphs(FIRA, 600)[::20]]


CASES = {
    "exact": lambda: list(K.exact_sets().values()),
    "counts1": lambda: K.unlike_neighbours(1), "counts63": lambda: K.unlike_neighbours(63), "counts64": lambda: K.unlike_neighbours(64),
    "counts65": lambda: K.unlike_neighbours(65), "counts129": lambda: K.unlike_neighbours(129),
    "sizes": _sizes,
    "noto": _noto,
}
_cache = {}


def case(name, oracle, vg):
    """(glyphs, restated glyphs, states, oracle bytes over the input, over the restated pieces), computed once"""
    if name not in _cache:
        glyphs = K.with_rects(CASES[name]())
        pieces, states = K.union_glyphs(glyphs)
        before, _ = oracle.sdf_render_batch(vg.make_batch(glyphs), oracle.PRECISE, 0)
        after, _ = oracle.sdf_render_batch(vg.make_batch(pieces), oracle.PRECISE, 0)
        _cache[name] = (glyphs, pieces, states, before, after)
    return _cache[name]


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def same_segments(seg_off, segs, pieces):
    assert list(np.diff(seg_off.astype(np.int64))) == [len(p[0]) for p in pieces]
    want = np.concatenate([p[0] for p in pieces]) if pieces else np.zeros((0, 4))
    assert segs.tobytes() == want.tobytes()   # bit for bit (-0.0 and 0.0 differ here)


def test_the_cases_are_the_intended_ones(oracle, vg):
    _, pieces, states, _, _ = case("sizes", oracle, vg)
    assert list(states) == [1] * 10 + [2, 3, 0]
    assert len(pieces[10][0]) == K.UNION_MAX_SEGMENTS + 1 and len(pieces[12][0]) == 9
    _, _, states, _, _ = case("counts129", oracle, vg)
    assert list(states[:4]) == [0, 1, 1, 0] and len(states) == 129
    _, _, states, before, after = case("noto", oracle, vg)
    assert len(states) == 38 + 30 and (states[:38] == 1).all() and (states[38:] == 0).all() and not np.array_equal(before, after)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_batch_union(oracle, vg, ctx, name, variant):
    glyphs, pieces, states, before, after = case(name, oracle, vg)
    ctx.set_variant(variant)
    db = ctx.upload(vg.make_batch(glyphs))
    try:
        ub, got_states = db.union()
        try:
            assert list(got_states) == list(states)
            same_segments(*ub.segments(), pieces)
            ub.launch()
            assert np.array_equal(ub.download(), after)
            st = ub.stats()
            assert st["n_glyphs"] == len(glyphs) and st["n_segments"] == sum(len(p[0]) for p in pieces)
        finally:
            ub.free()
        same_segments(*db.segments(), glyphs)   # the input batch is untouched ...
        db.launch()
        assert np.array_equal(db.download(), before)   # ... and still renders its old bytes
    finally:
        db.free()
        ctx.set_variant(0)


def _commands(vg, glyphs):
    """(cmd_off, cmds) of glyphs given as segments: every contour a move, its lines and a close, in f32 font units of 1/64 px"""
    parts, lens = [], []
    for g in glyphs:
        st = _stream(K.rings_of(g[0]), 64.0) if len(g[0]) else []
        parts.append(np.array([(c[1], c[2], c[3], c[4], c[5], c[6], c[0]) for c in st], dtype=vg.OUTLINE_CMD_DTYPE))
        lens.append(len(st))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), np.concatenate(parts)


@pytest.mark.parametrize("name", list(CASES))
def test_outlines_union_equals_the_batch_route(oracle, vg, ctx, name):
    """the same outlines as commands: the front-end's batch (32-byte records) through vgsdf_outlines_union against its own
    segments through vgsdf_batch_union, and both against the restatement.  Every glyph of every case goes, the empty ones, the
    one of exactly the limit and the one over it included; only a coordinate that is not finite cannot be a command
    (vgsdf_outlines_prepare refuses the batch): test_the_passes_on_records holds that state on this layout."""
    glyphs = [g for g in case(name, oracle, vg)[0] if np.isfinite(g[0]).all()]
    cmd_off, cmds = _commands(vg, glyphs)
    n = len(glyphs)
    c = vg.SdfContext(0)
    try:
        rects, ob, ns = c.outlines_prepare(cmd_off, cmds, np.full(n, 1.0 / 64.0), np.zeros(n))
        seg_off, segs = c.outlines_segments()
        plain = c.outlines_render()
        mine = [(segs[seg_off[g]:seg_off[g + 1]],) + ((int(rects[g]["x0"]), int(rects[g]["y0"]), int(rects[g]["w"]), int(rects[g]["h"]))
                                                    if rects[g]["has_raster"] else (0, 0, 0, 0)) for g in range(n)]
        # the front-end made what was meant: a glyph's segment count (so the limit and the one over it), no raster without segments
        assert [len(m[0]) for m in mine] == [len(g[0]) for g in glyphs]
        assert [int(r["has_raster"]) for r in rects] == [int(len(g[0]) > 0) for g in glyphs] and ob == sum(m[3] * m[4] for m in mine)
        pieces, states = K.union_glyphs(mine)
        got_states = c.outlines_union()
        u_off, u_segs = c.outlines_segments()
        out = c.outlines_render()
    finally:
        c.close()
    assert list(got_states) == list(states)
    if name == "sizes":
        assert [len(m[0]) for m in mine][9:11] == [K.UNION_MAX_SEGMENTS, K.UNION_MAX_SEGMENTS + 1] and list(states[9:11]) == [1, 2]
        assert pieces[10][0].tobytes() == mine[10][0].tobytes()   # over the limit: passed through bit for bit
    same_segments(u_off, u_segs, pieces)
    want, _ = oracle.sdf_render_batch(vg.make_batch(pieces), oracle.PRECISE, 0)
    assert np.array_equal(out, want)
    old, _ = oracle.sdf_render_batch(vg.make_batch(mine), oracle.PRECISE, 0)
    assert np.array_equal(plain, old)
    db = ctx.upload(vg.make_batch(mine))   # the batch route over the same segments
    try:
        ub, b_states = db.union()
        try:
            assert list(b_states) == list(got_states)
            b_off, b_segs = ub.segments()
            ub.launch()
            b_out = ub.download()
        finally:
            ub.free()
    finally:
        db.free()
    assert np.array_equal(b_off, u_off) and b_segs.tobytes() == u_segs.tobytes() and np.array_equal(b_out, out)


@pytest.mark.parametrize("stride", [4, 1])
def test_the_passes_on_records(oracle, vg, stride):
    """The count and the emit pass themselves (vgsdf_outline_union_count / _emit, the launchers the C ABI calls) over the `sizes`
    case laid out as 32-byte records {sx, sy, ex, ey} (seg_stride 4) in device memory of this test's own, in and out: every
    state on that layout, the glyph with a coordinate that is not finite (state 3: the vote, and the copy of the emit pass)
    and the one over the limit (state 2) included, bit for bit against the restatement."""
    import ctypes as C

    from versatiles_glyphs_rs_amd import device as D
    L = D.load_library()
    hip = C.CDLL("libamdhip64.so")   # (the runtime the library itself is linked against: already in the process)
    glyphs, pieces, states, _, _ = case("sizes", oracle, vg)
    n = len(glyphs)
    seg_off = np.concatenate([[0], np.cumsum([len(g[0]) for g in glyphs])]).astype(np.int64)
    desc = np.zeros(n, dtype=[("seg_off", "<u4"), ("n_seg", "<u4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<u4"), ("h", "<u4"), ("out_off", "<u8")])
    desc["seg_off"], desc["n_seg"] = seg_off[:-1], np.diff(seg_off)
    assert desc.itemsize == 32
    allseg = np.concatenate([g[0] for g in glyphs])
    n_in = len(allseg)
    want = np.concatenate([p[0] for p in pieces])
    total, guard = len(want), 64   # guard: segments behind the pieces that must stay as they are
    held = []

    def shared(shape, dtype):
        """page-locked host memory the kernels read and write in place (vgsdf_host_alloc), as an array"""
        nbytes = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 1)
        p = L.vgsdf_host_alloc(nbytes)
        assert p
        held.append(p)
        return np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=dtype, count=int(np.prod(shape))).reshape(shape), p

    def fields(p, count):
        """the four field pointers of `count` segments at p in this layout"""
        step = 8 if stride == 4 else 8 * count
        return [C.c_void_p(p + k * step) for k in range(4)]
    try:
        a_in, p_in = shared((n_in, 4) if stride == 4 else (4, n_in), np.float64)
        a_in[...] = allseg if stride == 4 else allseg.T
        a_desc, p_desc = shared((n,), desc.dtype)
        a_desc[...] = desc
        a_count, p_count = shared((n,), np.uint32)
        a_state, p_state = shared((n,), np.uint8)
        a_state[...] = 255
        a_first, p_first = shared((n_in,), np.uint32)
        a_off, p_off = shared((n + 1,), np.uint32)
        a_out, p_out = shared((total + guard, 4) if stride == 4 else (4, total + guard), np.float64)
        a_out[...] = -7.0
        vp, u32 = C.c_void_p, C.c_uint32
        L.vgsdf_outline_union_count.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        L.vgsdf_outline_union_emit.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp]
        assert L.vgsdf_outline_union_count(p_desc, n, *fields(p_in, n_in), stride, p_count, p_state, p_first, None) == 0
        assert hip.hipDeviceSynchronize() == 0
        assert list(a_state) == list(states) and list(a_count) == [len(p[0]) for p in pieces]
        a_off[...] = np.concatenate([[0], np.cumsum(a_count.astype(np.int64))])
        assert int(a_off[-1]) == total   # (the emit pass stores nothing outside [off[g], off[g + 1]) of a glyph)
        assert L.vgsdf_outline_union_emit(p_desc, n, *fields(p_in, n_in), stride, p_state, p_first, p_off, *fields(p_out, total + guard),
                                          stride, None) == 0
        assert hip.hipDeviceSynchronize() == 0
        got = (a_out if stride == 4 else a_out.T).copy()
        off = a_off.astype(np.int64)
    finally:
        for p in held:
            L.vgsdf_host_free(p)
    assert got[:total].tobytes() == want.tobytes()
    assert (got[total:] == -7.0).all()
    assert got[off[11]:off[12]].tobytes() == glyphs[11][0].tobytes() and states[11] == 3   # the non-finite glyph: copied as it stands


def test_an_empty_submission_after_a_union_forgets_the_union(vg):
    """prepare, union, then a submission of no glyphs: the context answers for the empty batch (one seg_off entry), not for the
    union of the batch before"""
    glyphs = K.with_rects([K.rect_set_segments("two_rects")] * 3)
    cmd_off, cmds = _commands(vg, glyphs)
    c = vg.SdfContext(0)
    try:
        c.outlines_prepare(cmd_off, cmds, np.full(3, 1.0 / 64.0), np.zeros(3))
        assert list(c.outlines_union()) == [1, 1, 1]
        assert len(c.outlines_segments()[0]) == 4
        rects, ob, ns = c.outlines_prepare(np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=vg.OUTLINE_CMD_DTYPE), np.zeros(0), np.zeros(0))
        assert (len(rects), ob, ns) == (0, 0, 0)
        seg_off = np.full(8, 0xFFFFFFFF, dtype=np.uint32)   # room to spare: what is written shows
        from versatiles_glyphs_rs_amd import device as D
        assert D.load_library().vgsdf_outlines_segments(c._h, seg_off.ctypes.data, None, None, None, None) == 0
        assert list(seg_off[1:]) == [0xFFFFFFFF] * 7
        assert list(c.outlines_union()) == []
    finally:
        c.close()
