"""GPU: the two flattening passes of the device front-end (outline_count / outline_emit_segments and wave_parallel_points in
csrc/outline_kernels.hip) on the command streams of test_flatten_shapes_host.py, where their split rules and the classes
every stream reaches are restated and witnessed on the CPU.

One batch holds every family (A cubic depth-bound edge, B cubic tree shapes, C coordinate bounds, D deep sequential cubics,
E wave composition, F ring state across 64-command steps, G non-monotone transforms), each from a wave boundary, so the
lanes the families were written for are the lanes they run on.  Checked per glyph: the segments byte for byte against the
oracle's RingBuilder x scale + shift, the rect against the one those segments give, each ring's point count against the
restated leaves, no refusal (error bit 2: a cubic broke its depth bound); the same batch in the packed upload form; bitmaps
of a few glyphs per family against the oracle's raster; and a CFF font of these shapes through FontManager with the device
front-end on and off."""
import numpy as np
import pytest

from test_flatten_shapes_host import assemble, batch_arrays, command_classes, ring_lengths, CFF_FIRST_CP, build_cff_font

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def oracle_segments(oracle, g):
    rings = oracle.build_rings(g.stream, cap=1 << 18, max_rings=1 << 12)
    segs = []
    for r in rings:
        p = r * g.scale
        p[:, 0] += g.shift
        p[:, 1] += 0.0
        segs.append(np.concatenate([p[:-1], p[1:]], axis=1))
    return np.concatenate(segs) if segs else np.zeros((0, 4))


def rect_of(segs):
    """Renderer::prepare_glyph on the points of those segments (renderer.rs:64-91): (has_raster, x0, y0, w, h, n_segments)"""
    if not len(segs):
        return (0, 0, 0, 0, 0, 0)
    p = np.concatenate([segs[:, :2], segs[:, 2:]])
    x0, y0 = p.min(0)
    x1, y1 = p.max(0)
    if x1 <= x0 and y1 <= y0:
        return (0, 0, 0, 0, 0, 0)
    ix0, iy0 = int(np.floor(x0)) - 3, int(np.floor(y0)) - 3
    return (1, ix0, iy0, int(np.ceil(x1)) + 3 - ix0, int(np.ceil(y1)) + 3 - iy0, len(segs))


def got_rect(r):
    if not r["has_raster"]:
        return (0, 0, 0, 0, 0, 0)
    return (1, int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]), int(r["n_segments"]))


@pytest.fixture(scope="module")
def batch(vg, oracle):
    glyphs, fam = assemble()
    cmd_off, cmds, scale, shift = batch_arrays(glyphs)
    cmds = np.array(cmds, dtype=vg.OUTLINE_CMD_DTYPE)
    want = [oracle_segments(oracle, g) for g in glyphs]
    return glyphs, fam, cmd_off, cmds, scale, shift, want


def check_glyphs(glyphs, want, rects, seg_off, segs):
    bad = []
    for i, g in enumerate(glyphs):
        got = segs[seg_off[i]:seg_off[i + 1]]
        if got.tobytes() != want[i].tobytes() or got_rect(rects[i]) != rect_of(want[i]):
            bad.append(g.name)
    assert not bad, (len(bad), bad[:10])


def test_segments_rects_and_point_counts(vg, ctx, batch):
    glyphs, fam, cmd_off, cmds, scale, shift, want = batch
    rects, out_bytes, n_segs = ctx.outlines_prepare(cmd_off, cmds, scale, shift)   # (refused batches raise)
    seg_off, segs = ctx.outlines_segments()
    check_glyphs(glyphs, want, rects, seg_off, segs)
    assert n_segs == sum(len(w) for w in want)
    # each ring's point count is what the restated leaves predict: the device's segments split into rings of those
    # counts, every ring ending where it started
    for i, g in enumerate(glyphs):
        lens = ring_lengths(g.stream, command_classes(g.stream, g.scale > 0))
        got = segs[seg_off[i]:seg_off[i + 1]]
        assert len(got) == sum(n - 1 for n in lens), g.name
        k = 0
        for n in lens:
            assert got[k + n - 2, 2:].tobytes() == got[k, :2].tobytes(), g.name
            k += n - 1
    assert set(fam) == set("ABCDEFG")


def test_packed_form_equals_the_record_form(vg, ctx, batch):
    """outlines_submit_packed (what FontManager uploads; the context pass expands the cubics' six floats): the same
    rects and segments.  (A capacity of one byte: the raster is not run.)"""
    glyphs, fam, cmd_off, cmds, scale, shift, want = batch
    dat_off, kinds, coords = vg.SdfContext.pack_outlines(cmd_off, cmds)
    c = vg.SdfContext(0)
    try:
        c.outlines_submit_packed(cmd_off, dat_off, kinds, coords, scale, shift, 1)
        rects, out, _, n_segs = c.outlines_wait()
        seg_off, segs = c.outlines_segments()
    finally:
        c.close()
    check_glyphs(glyphs, want, rects, seg_off, segs)
    assert n_segs == sum(len(w) for w in want)


def test_bitmaps_of_each_family(oracle, vg, ctx, batch):
    """a few glyphs of every family, one of them beyond 512 segments (command-derived chunk boxes), through
    outlines_render against the oracle's raster on the oracle's segments"""
    glyphs, fam, _, _, _, _, want = batch
    pick, per = [], {}
    for i, (g, f) in enumerate(zip(glyphs, fam)):
        r = rect_of(want[i])
        if not r[0] or r[3] * r[4] * max(r[5], 64) > 4.0e7:
            continue
        big = r[5] > 512
        key = (f, big)
        if per.get(key, 0) < (1 if big else 3):
            per[key] = per.get(key, 0) + 1
            pick.append(i)
    assert {f for f, _ in per} == set("ABCDEFG") and any(big for _, big in per)
    sub = [glyphs[i] for i in pick]
    cmd_off, cmds, scale, shift = batch_arrays(sub)
    rects, out_bytes, _ = ctx.outlines_prepare(cmd_off, np.array(cmds, dtype=vg.OUTLINE_CMD_DTYPE), scale, shift)
    out = ctx.outlines_render()
    off = 0
    for j, i in enumerate(pick):
        _, x0, y0, w, h, _ = rect_of(want[i])
        assert got_rect(rects[j]) == rect_of(want[i]), glyphs[i].name
        bm = oracle.sdf_render(want[i], x0, y0, w, h)
        assert np.array_equal(out[off:off + w * h].reshape(h, w), bm), glyphs[i].name
        off += w * h
    assert off == out_bytes


def test_cff_font_of_the_shapes_through_font_manager(oracle, vg):
    """the CFF font of families A, B, D and F: render_glyphs with the device front-end on and off gives the PBF bytes
    of oracle.render_block(..., PRECISE)"""
    pytest.importorskip("fontTools")
    font_bytes = build_cff_font()
    font = oracle.Font(font_bytes)
    blocks = sorted({int(cp) // 256 for cp in font.codepoints()})
    assert blocks[0] == CFF_FIRST_CP // 256
    want = None
    for fe in (True, False):
        m = vg.FontManager(True)
        m.set_device_front_end(fe)
        fid = m.add_font_data("Flatten Shapes", font_bytes)
        if want is None:
            want = {b: oracle.render_block([font], fid, b * 256, oracle.PRECISE)[0] for b in blocks}
        w = vg.DummyWriter()
        m.render_glyphs(w, vg.Renderer.new_precise(0))
        for b in blocks:
            assert w.files[f"{fid}/{b * 256}-{b * 256 + 255}.pbf"] == want[b], (fe, b)
