"""The five input forms of the device front-end, and every way their input can travel, on ONE glyph list and ONE context:
records (vgsdf_outlines_submit), packed and glyf as separate arrays and as one page-locked block in the order vgsdf.h
names for a single-copy upload, glyf fonts and command fonts named by (font, glyph id).

Everything is compared with the record form: rects, out_bytes and the bitmaps as bytes.  The runs with pbf_pre / pbf_fix
(the record form takes none) are compared among themselves and with the packed separate-array form: rects, the size of the
arena, vgsdf_outlines_pbf_positions, and every bitmap where the positions put it — which, taken in glyph order, are the
record form's bitmaps again.  No tolerance appears anywhere.

Sizes: 0, 1 and 257 glyphs (ids repeat): one past the 256-glyph workgroup of the kernels that expand or gather named
glyphs, several 64-lane waves of the per-glyph kernels.  One batch of 257 carries a scale of +inf on a glyph without outline:
every form then takes the separate context pass.

The last case pins a sequence: a page-locked packed block whose dat_off is not monotone is refused (VGSDF_E_ARG) after its
upload was enqueued; block and output buffer stay allocated; the corrected block on the same context renders what the
record form renders.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_front_end import _varint_len
from test_gpu_resident_fonts import _glyf_subset

pytestmark = pytest.mark.gpu

CAPACITY = 1 << 20
E_ARG = -1


# ---- the single-copy blocks, restated from include/vgsdf.h ----

def _up(v, a):
    return (v + a - 1) // a * a


def _packed_block_offsets(n, n_cmds, n_floats, pbf):
    """scale | shift_x | cmd_off | dat_off | (pad to 8) | coords | kinds [| (pad to 4) | pbf_pre | pbf_fix]"""
    at = {"scale": 0, "shift_x": 8 * n, "cmd_off": 16 * n}
    at["dat_off"] = at["cmd_off"] + 4 * (n + 1)
    at["coords"] = _up(at["dat_off"] + 4 * (n + 1), 8)
    at["kinds"] = at["coords"] + 4 * n_floats
    at["pbf_pre"] = _up(at["kinds"] + n_cmds, 4)
    at["pbf_fix"] = at["pbf_pre"] + 4 * n
    return at, (at["pbf_fix"] + n if pbf else at["kinds"] + n_cmds)


def _glyf_block_offsets(n, n_parts, n_bytes, pbf):
    """scale | shift_x | cmd_off | (pad to 8) | parts | bytes [| pbf_pre | pbf_fix]"""
    at = {"scale": 0, "shift_x": 8 * n, "cmd_off": 16 * n}
    at["parts"] = _up(at["cmd_off"] + 4 * (n + 1), 8)
    at["bytes"] = at["parts"] + 48 * n_parts
    at["pbf_pre"] = at["bytes"] + n_bytes
    at["pbf_fix"] = at["pbf_pre"] + 4 * n
    return at, (at["pbf_fix"] + n if pbf else at["pbf_pre"])


class _Block:
    """arrays placed in one block from vgsdf_host_alloc; ptr(name): where an array lies"""

    def __init__(self, L, offsets, size, arrays):
        self.L, self.at = L, offsets
        self.base = L.vgsdf_host_alloc(max(size, 16))
        assert self.base
        self.mem = np.frombuffer((C.c_uint8 * max(size, 16)).from_address(self.base), dtype=np.uint8)
        for name, a in arrays.items():
            self.put(name, a)

    def put(self, name, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.mem[self.at[name]:self.at[name] + len(raw)] = raw

    def ptr(self, name):
        return self.base + self.at[name]

    def free(self):
        self.mem = None
        self.L.vgsdf_host_free(self.base)


# ---- the glyph list in every form ----

@pytest.fixture(scope="module")
def world(vg):
    from conftest import FIRA
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name("Font", [FIRA])
    o = mgr.record_outlines(fid)
    g = mgr.record_glyf_parts(fid)
    r = mgr.record_resident(fid)
    rc = mgr.record_resident_commands(fid)
    for other in (g, r, rc):
        assert np.array_equal(other["ids"], o["ids"])
        assert np.array_equal(other["scale"], o["scale"]) and np.array_equal(other["shift_x"], o["shift_x"])
    assert r["n_files"] == rc["n_files"] == 1
    d, dc = mgr.resident_font_desc(fid, 0), mgr.command_font_desc(fid, 0)
    ctx = vg.SdfContext(0)
    font = ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"])
    cfont = ctx.font_create_commands(dc["cmd_off"], dc["dat_off"], dc["kinds"], dc["coords"])
    yield {"vg": vg, "L": vg.device.load_library(), "ctx": ctx, "o": o, "g": g, "r": r, "rc": rc, "font": font, "cfont": cfont}
    font.free()
    cfont.free()
    ctx.close()


def _selection(o, n, with_inf):
    """indices into the recorded font (repeats, any order), scale and shift of the batch"""
    counts = np.diff(o["cmd_off"].astype(np.int64))
    empty, drawn = np.flatnonzero(counts == 0), np.flatnonzero(counts > 0)
    assert len(empty) >= 1 and len(drawn) > 1000
    if n == 0:
        sel = np.zeros(0, np.int64)
    elif n == 1:
        sel = drawn[[len(drawn) // 2]]
    else:
        rng = np.random.default_rng(257)
        sel = rng.choice(drawn, n)                 # (with replacement: ids repeat)
        sel[[5, n - 1]] = sel[0]
        sel[[64, 200]] = empty[0]                  # glyphs without outline, one of them at a wave's first lane
    scale, shift = o["scale"][sel].copy(), o["shift_x"][sel].copy()
    if with_inf:
        scale[200] = np.inf
    return sel, scale, shift


def _forms(w, sel, scale, shift):
    """the glyph list as the arguments of every form"""
    o, g = w["o"], w["g"]
    off = o["cmd_off"].astype(np.int64)
    cmd_off = np.concatenate([[0], np.cumsum(off[sel + 1] - off[sel])]).astype(np.uint32)
    cmds = np.concatenate([o["cmds"][off[i]:off[i + 1]] for i in sel]) if len(sel) else o["cmds"][:0]
    dat_off, kinds, coords = w["vg"].SdfContext.pack_outlines(cmd_off, cmds)
    slot_off, parts, store, _, _ = _glyf_subset(g, sel)
    return {"records": (cmd_off, cmds), "packed": (cmd_off, dat_off, kinds, coords), "glyf": (slot_off, parts, store),
            "scale": scale, "shift": shift, "sel": sel}


def _pbf_arrays(w, sel):
    ids, adv = w["o"]["ids"][sel], w["o"]["advances"][sel]
    fix = np.array([(1 + _varint_len(int(i))) | ((1 + _varint_len(int(a))) << 4) for i, a in zip(ids, adv)], dtype=np.uint8)
    pre = np.zeros(len(sel), dtype=np.uint32)
    if len(sel):
        pre[0] = 36
    if len(sel) > 129:
        pre[128], pre[129] = 37, 77                # "block" starts
    return pre, fix


def _raw_submit(w, name, co, n, keep):
    """a submission through the C ABI itself (the block forms: the binding's wrappers take separate arrays); the output
    buffer and the bookkeeping are those of the wrappers, so that the context's outlines_wait collects it"""
    L, ctx = w["L"], w["ctx"]
    host = L.vgsdf_host_alloc(CAPACITY)
    assert host
    rc = getattr(L, name)(ctx._h, C.byref(co), host, CAPACITY)
    if rc != 0:
        L.vgsdf_host_free(host)
        ctx._check(rc)
    ctx._inflight = (keep, host, CAPACITY, n)


def _collect(ctx, pbf):
    rects, out, ob, _ = ctx.outlines_wait()
    assert out is not None
    if pbf and len(rects) == 0:                    # (nothing was laid out: there are no positions to ask for)
        return rects, out, ob, np.zeros(0, np.uint64)
    return rects, out, ob, (ctx.outlines_pbf_positions() if pbf else None)


def _submit_form(w, f, form, pbf):
    """form: records | packed | packed_block | glyf | glyf_block | resident | commands -> (rects, out, out_bytes, positions)"""
    dev, ctx, L = w["vg"].device, w["ctx"], w["L"]
    n, scale, shift = len(f["sel"]), f["scale"], f["shift"]
    kw = dict(zip(("pbf_pre", "pbf_fix"), pbf)) if pbf else {}
    block = None
    if form == "records":
        ctx.outlines_submit(*f["records"], scale, shift, CAPACITY)
    elif form == "packed":
        ctx.outlines_submit_packed(*f["packed"], scale, shift, CAPACITY, **kw)
    elif form == "glyf":
        ctx.outlines_submit_glyf(*f["glyf"], scale, shift, CAPACITY, **kw)
    elif form == "resident":
        ctx.outlines_submit_resident([w["font"]], w["r"]["font_of"][f["sel"]], w["r"]["glyph_id"][f["sel"]], scale, shift, CAPACITY, **kw)
    elif form == "commands":
        ctx.outlines_submit_resident([w["cfont"]], w["rc"]["font_of"][f["sel"]], w["rc"]["glyph_id"][f["sel"]], scale, shift, CAPACITY, **kw)
    elif form == "packed_block":
        block, co = _packed_block(L, dev, f, pbf)
        _raw_submit(w, "vgsdf_outlines_submit_packed", co, n, block)
    elif form == "glyf_block":
        cmd_off, parts, store = f["glyf"]
        at, size = _glyf_block_offsets(n, len(parts), len(store), bool(pbf))
        arrays = {"scale": scale, "shift_x": shift, "cmd_off": cmd_off, "parts": parts, "bytes": store}
        if pbf:
            arrays.update(pbf_pre=pbf[0], pbf_fix=pbf[1])
        block = _Block(L, at, size, arrays)
        co = dev._COutlinesGlyf(n, len(parts), len(store), block.ptr("cmd_off"), block.ptr("parts"), block.ptr("bytes"), block.ptr("scale"),
                                block.ptr("shift_x"), block.ptr("pbf_pre") if pbf else None, block.ptr("pbf_fix") if pbf else None)
        _raw_submit(w, "vgsdf_outlines_submit_glyf", co, n, block)
    else:
        raise AssertionError(form)
    try:
        return _collect(ctx, bool(pbf))
    finally:
        if block is not None:
            block.free()


def _packed_block(L, dev, f, pbf, dat_off=None):
    cmd_off, good_dat_off, kinds, coords = f["packed"]
    n = len(f["sel"])
    at, size = _packed_block_offsets(n, len(kinds), len(coords), bool(pbf))
    arrays = {"scale": f["scale"], "shift_x": f["shift"], "cmd_off": cmd_off, "dat_off": good_dat_off if dat_off is None else dat_off,
              "coords": coords, "kinds": kinds}
    if pbf:
        arrays.update(pbf_pre=pbf[0], pbf_fix=pbf[1])
    block = _Block(L, at, size, arrays)
    co = dev._COutlinesPacked(n, block.ptr("cmd_off"), block.ptr("dat_off"), block.ptr("kinds"), block.ptr("coords"), block.ptr("scale"),
                              block.ptr("shift_x"), block.ptr("pbf_pre") if pbf else None, block.ptr("pbf_fix") if pbf else None)
    return block, co


def _bitmaps_of_arena(rects, arena, at):
    """the bitmaps where the positions put them, in glyph order (the bytes between them are the caller's)"""
    pieces = []
    for pos, r in zip(at, rects):
        if r["has_raster"]:
            size = int(r["w"]) * int(r["h"])
            assert int(pos) + size <= len(arena)
            pieces.append(arena[int(pos):int(pos) + size])
    return np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)


OTHER_FORMS = ("packed", "packed_block", "glyf", "glyf_block", "resident", "commands")


@pytest.mark.parametrize("n,with_inf", [(0, False), (1, False), (257, False), (257, True)], ids=["0", "1", "257", "257_inf_scale"])
def test_every_form_and_travel_path_renders_what_the_record_form_renders(world, n, with_inf):
    w = world
    sel, scale, shift = _selection(w["o"], n, with_inf)
    f = _forms(w, sel, scale, shift)
    rects, bitmaps, out_bytes, _ = _submit_form(w, f, "records", None)
    assert len(rects) == n and out_bytes == len(bitmaps)
    if n:
        assert int(rects["has_raster"].sum()) >= (1 if n == 1 else n - 8) and out_bytes > 0
    if n == 257:
        assert not rects["has_raster"][[64, 200]].any()
    for form in OTHER_FORMS:
        r2, b2, ob2, _ = _submit_form(w, f, form, None)
        assert r2.tobytes() == rects.tobytes(), form
        assert ob2 == out_bytes and b2.tobytes() == bitmaps.tobytes(), form
    pbf = _pbf_arrays(w, sel)
    want = None
    for form in OTHER_FORMS:                       # (the first: the packed separate-array form)
        r2, arena, ob2, at = _submit_form(w, f, form, pbf)
        assert r2.tobytes() == rects.tobytes() and len(at) == n and len(arena) == ob2, form
        got = (ob2, at.tobytes(), _bitmaps_of_arena(r2, arena, at).tobytes())
        if want is None:
            want = got
            assert got[2] == bitmaps.tobytes() and (ob2 > out_bytes or n == 0)
        assert got == want, form


def test_a_refused_block_leaves_the_context_ready_for_the_corrected_one(world):
    w = world
    L, ctx, dev = w["L"], w["ctx"], w["vg"].device
    sel, scale, shift = _selection(w["o"], 257, False)
    f = _forms(w, sel, scale, shift)
    rects, bitmaps, out_bytes, _ = _submit_form(w, f, "records", None)
    good = f["packed"][1]
    bad = good.copy()
    bad[3] = bad[4] + 2                            # dat_off[4] < dat_off[3]; first and last entries as they were
    assert bad[0] == 0 and bad[-1] == good[-1] and bad[4] < bad[3]
    block, co = _packed_block(L, dev, f, None, dat_off=bad)
    out = L.vgsdf_host_alloc(CAPACITY)
    assert out
    try:
        rc = L.vgsdf_outlines_submit_packed(ctx._h, C.byref(co), out, CAPACITY)
        assert rc == E_ARG and b"monotone" in L.vgsdf_last_error(ctx._h)
        # block and output buffer stay allocated; the corrected block, same context, same buffers
        block.put("dat_off", good)
        ctx._check(L.vgsdf_outlines_submit_packed(ctx._h, C.byref(co), out, CAPACITY))
        r2 = np.zeros(len(sel), dtype=dev.RECT_DTYPE)
        ob, ns, done = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        ctx._check(L.vgsdf_outlines_wait(ctx._h, r2.ctypes.data, C.byref(ob), C.byref(ns), C.byref(done)))
        assert done.value == 1 and int(ob.value) == out_bytes
        got = np.frombuffer((C.c_uint8 * CAPACITY).from_address(out), dtype=np.uint8, count=out_bytes)
        assert r2.tobytes() == rects.tobytes() and got.tobytes() == bitmaps.tobytes()
    finally:
        L.vgsdf_host_free(out)
        block.free()
