"""GPU: the device front-end (csrc/outline_kernels.hip, csrc/outline_plan_kernels.hip) across its size-dependent branches, at the C ABI.

A. Plan regimes.  Noto Sans Regular, recorded with the oracle's reader and tiled cyclically to n glyphs, through every
   submission form.  n crosses the plan's instances (outline_plan<4, true> up to 4096 glyphs with in-place PBF,
   <8, true> up to 8192, <8, false> above: every glyph placed twice), its run lengths per thread (1024 / 1025, 4096 / 4097,
   8192 / 8193), the span budget (8 below 2048 glyphs, 16 from there), and, on one context in ascending then descending
   order, the raster grid guessed from the previous batch both holding and too small.  Expected values come from the
   committed goldens only: every bitmap's SHA-256 and every rect follow from glyphs_noto_regular.csv.

C. Chunk boxes from the commands (chunk_boxes_of_glyph).  Stacked rings built as command streams: segment counts on both
   sides of "boxes at all" (512 / 513), of a chunk boundary (768 / 769) and of the 256-chunk LDS limit (65 536 / 65 537),
   rings starting on and one segment before a chunk boundary, closes that append point 0 in a later chunk, closes by
   equality and within the close rule's epsilon, single curves whose points cover several chunks, open rings, many rings;
   at a positive, a power-of-two and a negative scale (boxes from the transformed points), with fractional shifts.  Three
   witnesses per glyph: the oracle's rings, the oracle's raster, and vgsdf_render_batch (exact segment boxes) on the
   segments the device produced."""
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import NOTO
from test_golden_cpu import golden_rows
from test_gpu_front_end import record, restate_pbf_layout

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

SIZES = (1, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 8191, 8192, 8193, 20000)
FORMS = ("into", "prepare", "packed", "pbf")
M, L, Q, C3, Z = 0, 1, 2, 3, 4


# ---------------------------------------------------------------------------------------------------------------------
# A. plan regimes
# ---------------------------------------------------------------------------------------------------------------------

class Tiled:
    """n glyphs: the recorded entries repeated cyclically (each keeps its scale and shift), with what the goldens say
    about each of them"""

    def __init__(self, vg, src, n, extra=None):
        cmd_off, cmds, scale, shift, exp = src
        e = len(scale)
        idx = (np.arange(n) + int(np.argmax(exp["has"]))) % e   # (from the first entry with a bitmap: n = 1 renders one)
        parts = [cmds[cmd_off[i]:cmd_off[i + 1]] for i in idx]
        lens = (cmd_off[1:] - cmd_off[:-1])[idx].astype(np.int64)
        self.scale, self.shift = scale[idx].copy(), shift[idx].copy()
        self.has = exp["has"][idx].copy()
        self.rect = exp["rect"][idx].copy()          # x0, y0, w, h, n_segments
        self.sha = [exp["sha"][i] for i in idx]
        if extra is not None:                        # one glyph of its own at the end: (cmds, scale, shift)
            xc, xs, xh = extra
            parts.append(xc)
            lens = np.append(lens, len(xc))
            self.scale, self.shift = np.append(self.scale, xs), np.append(self.shift, xh)
            self.has = np.append(self.has, True)
            self.rect = np.concatenate([self.rect, np.zeros((1, 5), np.int64)])
            self.sha.append(None)                    # (checked against the oracle by the caller)
        self.n = len(self.scale)
        self.cmds = np.concatenate(parts) if parts else np.zeros(0, dtype=vg.OUTLINE_CMD_DTYPE)
        self.cmd_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        self.dat_off, self.kinds, self.coords = vg.SdfContext.pack_outlines(self.cmd_off, self.cmds)
        px = np.where(self.has, self.rect[:, 2] * self.rect[:, 3], 0)
        self.out_bytes = int(px.sum())
        self.n_segs = int(np.where(self.has, self.rect[:, 4], 0).sum())
        # in-place PBF: id / advance varints of 1..3 bytes in a pattern unlike the glyphs', block starts (pbf_pre != 0) at
        # every 256th glyph, at run boundaries of the plan's threads and inside runs
        g = np.arange(self.n)
        self.fix = ((2 + g % 3) | ((2 + (g // 3) % 3) << 4)).astype(np.uint8)
        self.pre = np.zeros(self.n, dtype=np.uint32)
        run = max(1, -(-self.n // 1024))
        self.pre[::256] = 36
        self.pre[np.arange(0, self.n, run)[::7]] = 37
        if run > 1:
            inside = np.arange(run // 2, self.n, run)[3::11]
            self.pre[inside] = 6 + (inside % 50).astype(np.uint32)
        self.pre[-1] = 77


def check_rects(t, rects, skip_last=False):
    k = t.n - 1 if skip_last else t.n
    got_has = rects["has_raster"][:k].astype(bool)
    assert np.array_equal(got_has, t.has[:k]), np.flatnonzero(got_has != t.has[:k])[:8]
    got = np.stack([rects[f][:k].astype(np.int64) for f in ("x0", "y0", "w", "h", "n_segments")], 1)
    bad = np.flatnonzero((got != t.rect[:k]).any(1) & t.has[:k])
    assert bad.size == 0, (bad[:8], got[bad[:3]], t.rect[bad[:3]])


def check_packed(t, rects, out, last=None):
    """bitmaps packed back to back in glyph order: each one's SHA-256 is the golden one (the last glyph against `last`)"""
    assert out is not None and len(out) == t.out_bytes + (0 if last is None else last.size)
    off, bad = 0, []
    for g in np.flatnonzero(t.has):
        px = int(rects[g]["w"]) * int(rects[g]["h"])
        if t.sha[g] is None:
            assert np.array_equal(out[off:off + px].reshape(last.shape), last), g
        elif hashlib.sha256(out[off:off + px].tobytes()).hexdigest() != t.sha[g]:
            bad.append(int(g))
        off += px
    assert off == len(out) and not bad, (len(bad), bad[:8])


def run_form(vg, c, t, form, last=None):
    """one submission of `t` in `form` on context `c`, checked; -> the packed bitmaps"""
    extra_px = 0 if last is None else last.size
    ob_want, seg_want = t.out_bytes + extra_px, None if last is not None else t.n_segs
    if form == "into":
        rects, out, ob, ns = c.outlines_render_into(t.cmd_off, t.cmds, t.scale, t.shift, ob_want + 1000)
    elif form == "prepare":
        rects, ob, ns = c.outlines_prepare(t.cmd_off, t.cmds, t.scale, t.shift)
        out = c.outlines_render()
    else:
        c.outlines_submit_packed(t.cmd_off, t.dat_off, t.kinds, t.coords, t.scale, t.shift, ob_want + 64)
        rects, out, ob, ns = c.outlines_wait()
    check_rects(t, rects, skip_last=last is not None)
    assert ob == ob_want and (seg_want is None or ns == seg_want), (form, t.n, ob, ns)
    check_packed(t, rects, out, last)
    if form != "pbf":
        return out
    packed = out
    want_at, total = restate_pbf_layout(rects, t.pre, t.fix)
    for cap in (total + 64, 64):                     # 64: the arena does not fit, the bitmaps come from the second launches
        c.outlines_submit_packed(t.cmd_off, t.dat_off, t.kinds, t.coords, t.scale, t.shift, cap, pbf_pre=t.pre, pbf_fix=t.fix)
        r2, arena, ob2, ns2 = c.outlines_wait()
        assert r2.tobytes() == rects.tobytes() and ns2 == ns and ob2 == total, (t.n, cap)
        assert (arena is None) == (cap == 64), (t.n, cap)
        if arena is None:
            arena = c.outlines_render()
        at = c.outlines_pbf_positions()
        assert [int(v) for v in at] == want_at, (t.n, cap)
        poff = 0
        for g in np.flatnonzero(rects["has_raster"]):
            px = int(rects[g]["w"]) * int(rects[g]["h"])
            assert arena[want_at[g]:want_at[g] + px].tobytes() == packed[poff:poff + px].tobytes(), (t.n, cap, g)
            poff += px
        assert poff == len(packed)
    return packed


@pytest.fixture(scope="module")
def noto_src(vg, oracle):
    """every code point of Noto Sans Regular (glyphs_noto_regular.csv, empty glyphs included) recorded with the oracle's
    reader, and the expected rect / SHA-256 of each from the CSV"""
    rows = golden_rows("noto_regular")
    cmd_off, cmds, scale, shift, ids = record(vg, oracle.Font(NOTO), [int(r["codepoint"]) for r in rows])
    assert ids == [int(r["codepoint"]) for r in rows]
    has = np.array([int(r["bitmap_size"]) > 0 for r in rows])
    rect = np.zeros((len(rows), 5), np.int64)
    for i, r in enumerate(rows):
        w, h = int(r["width"]) + 6, int(r["height"]) + 6
        rect[i] = (int(r["left"]) - 3, int(r["top"]) + 27 - h, w, h, int(r["n_segments"]))
    assert 2900 < len(rows) < 3100 and 0 < (~has).sum()
    return cmd_off, cmds, scale, shift, {"has": has, "rect": rect, "sha": [r["sha256"] for r in rows]}


@pytest.fixture(scope="module")
def tiled(vg, noto_src):
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = Tiled(vg, noto_src, n)
        return cache[n]
    return get


def test_the_restated_expectations_hold_for_the_recorded_entries(oracle, noto_src):
    """(the expected rects of this module are the oracle's prepare_glyph for the entries tiled)"""
    _, _, _, _, exp = noto_src
    font = oracle.Font(NOTO)
    for i, r in enumerate(golden_rows("noto_regular")[::7]):
        info, _ = font.prepare_glyph(int(r["codepoint"]))
        assert bool(info.has_bitmap) == exp["has"][i * 7]
        if info.has_bitmap:
            assert (info.x0, info.y0, info.w, info.h, info.n_segments) == tuple(exp["rect"][i * 7])


def test_sizes_ascending_then_descending_on_one_context(vg, tiled):
    """one context per form sees every size in ascending then descending order: the one-submission forms guess the raster's
    grid from the previous batch (1.5 x its spans + 256), so growing steps (1 -> 1023, 2048 -> 4095, 4097 -> 8191,
    8193 -> 20 000) run the second launches and the others run behind the plan"""
    ctxs = {f: vg.SdfContext(0) for f in FORMS}
    try:
        for n in SIZES + SIZES[::-1]:
            for f in FORMS:
                run_form(vg, ctxs[f], tiled(n), f)
    finally:
        for c in ctxs.values():
            c.close()


@pytest.mark.parametrize("n", SIZES)
def test_each_size_on_a_fresh_context(vg, tiled, n):
    """no previous batch: the first submission of a context guesses the whole work-list capacity"""
    for f in FORMS:
        c = vg.SdfContext(0)
        try:
            run_form(vg, c, tiled(n), f)
        finally:
            c.close()


def test_largest_size_with_the_brute_force_variant(vg, tiled):
    """vgsdf_set_variant(1): no raster enqueued behind the plan, every bitmap from the launches after the read-back"""
    c = vg.SdfContext(0)
    try:
        c.set_variant(1)
        for f in FORMS:
            run_form(vg, c, tiled(SIZES[-1]), f)
    finally:
        c.close()


WIDE = [(0, 0, 0, 0, 0, 0, M), (0, 0, 0, 0, 60000, 0, L), (0, 0, 0, 0, 60000, 1000, L), (0, 0, 0, 0, 0, 1000, L), (0,) * 6 + (Z,)]


def _oracle_bitmap(oracle, stream, scale, shift, rect):
    segs = []
    for r in oracle.build_rings([(k[6],) + tuple(k[:6]) for k in stream]):
        p = r * scale
        p[:, 0] += shift
        p[:, 1] += 0.0
        segs.append(np.concatenate([p[:-1], p[1:]], axis=1))
    return oracle.sdf_render(np.concatenate(segs), int(rect["x0"]), int(rect["y0"]), int(rect["w"]), int(rect["h"]))


@pytest.mark.parametrize("n", (4096, 8192, 8193))
def test_a_brute_force_class_glyph_last(oracle, vg, noto_src, n):
    """n glyphs, the last too wide for the span kernel's winding histogram (test_one_submission_with_a_glyph_for_the_brute_
    force_class): the raster behind the plan must not run and the second launches give the goldens and the oracle's bytes"""
    t = Tiled(vg, noto_src, n - 1, extra=(np.array(WIDE, dtype=vg.OUTLINE_CMD_DTYPE), 24.0 / 1000.0, 0.25))
    c = vg.SdfContext(0)
    try:
        rects, _, _ = c.outlines_prepare(t.cmd_off, t.cmds, t.scale, t.shift)
        r = rects[-1]
        assert int(r["has_raster"]) == 1 and int(r["w"]) > 1400
        last = _oracle_bitmap(oracle, WIDE, 24.0 / 1000.0, 0.25, r)
        for f in FORMS:
            run_form(vg, c, t, f, last=last)
    finally:
        c.close()


TRACE_CODE = r'''
import sys
sys.path.insert(0, "tests")
from conftest import load_product, NOTO
from oracle import oracle as O
from test_gpu_front_end import record
vg = load_product()
font = O.Font(NOTO)
cps = [int(c) for c in font.codepoints() if 0x41 <= c <= 0xFFFF]   # (from "A": the first batch has a bitmap, so spans)
c = vg.SdfContext(0)
for n in (1, 1023, 1023):
    cmd_off, cmds, scale, shift, _ = record(vg, font, cps[:n])
    rects, out, ob, ns = c.outlines_render_into(cmd_off, cmds, scale, shift, 1 << 24)
    assert out is not None and len(out) == ob and int(rects[0]["has_raster"]) == 1
    print("[test] batch of", n, file=sys.stderr, flush=True)
c.close()
print("done")
'''


def test_trace_reports_both_outcomes_of_the_guess(vg):
    """VGSDF_TRACE=1 (read once per process, so in a child): 1 -> 1023 glyphs on one context is a guess too small, 1023
    again a guess that holds"""
    env = dict(os.environ, VGSDF_TRACE="1")
    cp = subprocess.run([sys.executable, "-c", TRACE_CODE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and cp.stdout.strip().endswith("done"), cp.stderr[-2000:]
    outcome = [ln for ln in cp.stderr.splitlines() if "one submission" in ln]
    assert len(outcome) == 3 and "guess too small: second launches" in outcome[1], cp.stderr[-3000:]
    assert "one submission, " in outcome[2], cp.stderr[-3000:]


@pytest.mark.parametrize("n", (2047, 2048))
def test_host_plan_at_the_span_budget_edge(vg, tiled, n):
    """the span budget changes from 8 to 16 at 2048 glyphs in the device's plan and in the host's: the segments the front-end
    produced, planned on the host (vgsdf_render_batch, boxes from the segments), give the front-end's bytes"""
    t = tiled(n)
    c = vg.SdfContext(0)
    try:
        rects, ob, _ = c.outlines_prepare(t.cmd_off, t.cmds, t.scale, t.shift)
        out = c.outlines_render()
        seg_off, segs = c.outlines_segments()
        glyphs = [(segs[seg_off[g]:seg_off[g + 1]], int(rects[g]["x0"]), int(rects[g]["y0"]), int(rects[g]["w"]), int(rects[g]["h"]))
                  for g in np.flatnonzero(rects["has_raster"])]
        got = c.render_batch(vg.make_batch(glyphs))
        assert len(out) == ob and got.tobytes() == out.tobytes()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. chunk boxes from the commands
# ---------------------------------------------------------------------------------------------------------------------

PITCH = 17.0                                         # px between stacked rings: most chunks far from most spans


def _ring_px(n_seg, k, cx=8.0):
    """n_seg points of ring k of a stack (px, before the glyph's scale): a wobbly circle of radius ~5 px, 17 px above ring
    k - 1; closed by Ring::close appending point 0 it has n_seg segments"""
    a = np.linspace(0, 2 * np.pi, n_seg, endpoint=False)
    r = 5.0 * (1 + 0.25 * np.sin(3 * a + k))
    pts = np.stack([cx + r * np.cos(a), 10.0 + PITCH * k + r * np.sin(a)], 1)
    return pts[::-1] if k % 2 else pts


def _stream(rings_px, unit, open_last=False, eps_last=()):
    """command stream (oracle order: kind, x1, y1, x2, y2, x, y) of rings given in px; unit: font units per px.
    eps_last: {ring: "equal" | "eps"}: rings moved to x = 0 at their first point and given one more point, equal to the
    first ("equal") or 1e-17 font units right of it ("eps": within the close rule's absolute f64 epsilon) -- nothing is
    appended to them, they keep n_seg segments"""
    st = []
    for i, pts in enumerate(rings_px):
        fu = (pts * unit).astype(np.float32)
        if i in eps_last:
            fu[:, 0] -= fu[0, 0]                     # the first point's x is exactly 0
            fu = np.concatenate([fu, fu[:1]])
            fu[-1, 0] = np.float32(1e-17) if eps_last[i] == "eps" else np.float32(0.0)
        st.append((M, 0, 0, 0, 0, float(fu[0, 0]), float(fu[0, 1])))
        st += [(L, 0, 0, 0, 0, float(x), float(y)) for x, y in fu[1:]]
        if not (open_last and i == len(rings_px) - 1):
            st.append((Z, 0, 0, 0, 0, 0, 0))
    return st


def _column_ring(n_seg, unit, top=400.0):
    """a tall zig-zag ring of n_seg segments: point 0 at the top left, n_seg - 1 points down the right side, the last at the
    bottom left; Ring::close appends point 0, so the last segment (in the ring's last chunk) runs up the whole left side"""
    ys = np.linspace(top, 10.0, n_seg)
    pts = [(0.0, top)] + [(6.0 + 2.0 * (j % 2), ys[j]) for j in range(1, n_seg - 1)] + [(0.0, 10.0)]
    fu = (np.array(pts) * unit).astype(np.float32)
    return [(M, 0, 0, 0, 0, float(fu[0, 0]), float(fu[0, 1]))] + [(L, 0, 0, 0, 0, float(x), float(y)) for x, y in fu[1:]] + \
        [(Z, 0, 0, 0, 0, 0, 0)]


def box_streams(unit):
    """(name, stream, expected segment count or None) in font units for `unit` font units per px"""
    out = []
    for sizes in ((256, 256), (255, 258), (256, 255, 257), (257, 255, 257)):          # 512, 513, 768, 769
        out.append((f"rings{sizes}", _stream([_ring_px(s, k) for k, s in enumerate(sizes)], unit), sum(sizes)))
    out.append(("65536", _stream([_ring_px(4096, k) for k in range(16)], unit), 65536))
    out.append(("65537", _stream([_ring_px(4096 + (k == 9), k) for k in range(16)], unit), 65537))
    # closes: Ring::close appends point 0 and the appended segment lies chunks after point 0's command
    out.append(("column600", _column_ring(600, unit), 600))
    out.append(("column1100", _column_ring(1100, unit) + _column_ring(300, unit, top=200.0), 1400))
    # last point == first / within epsilon of it (nothing appended), beside an appended close, spanning chunk boundaries
    r = [_ring_px(300, 0), _ring_px(300, 1), _ring_px(300, 2)]
    out.append(("eq-eps", _stream(r, unit, eps_last={0: "equal", 1: "eps"}), 900))
    # one command whose points cover several chunks: a quad_to / curve_to of high curvature for the scale
    h = 150.0 * unit
    out.append(("quad", [(M, 0, 0, 0, 0, 0.0, 0.0), (Q, 0.05 * h, 3.0 * h, 0, 0, 0.1 * h, 0.0), (Z,) + (0,) * 6], None))
    out.append(("cubic", [(M, 0, 0, 0, 0, 0.0, 0.0), (C3, 2.0 * h, 3.0 * h, -1.2 * h, 3.0 * h, 0.8 * h, 0.0),
                          (L, 0, 0, 0, 0, 0.4 * h, -0.3 * h), (Z,) + (0,) * 6], None))
    # a ring left open (the stream ends without a close) below closed ones; a glyph of many small rings
    out.append(("open", _stream([_ring_px(200, k) for k in range(4)], unit, open_last=True), 800))
    many = [_ring_px(12, k // 3, cx=8.0 + 14.0 * (k % 3)) for k in range(3 * 24)]
    out.append(("many", _stream(many, unit), 12 * 72))
    return out


# scale (font units -> px) and shift_x: 24/1000, a power of two, mirrored (boxes from the transformed points), fractional shifts
BOX_SCALES = ((24.0 / 1000.0, 0.0), (1.0 / 32.0, -0.21), (-24.0 / 1000.0, 0.125), (24.0 / 1000.0, 0.37))


@pytest.fixture(scope="module")
def box_batch(vg, oracle):
    """every stream at every scale -> (names, cmd_off, cmds, scale, shift, the oracle's segments per glyph)"""
    names, cmds, cmd_off, scale, shift, want = [], [], [0], [], [], []
    for sc, dx in BOX_SCALES:
        for name, st, n_seg in box_streams(1.0 / abs(sc)):
            rings = oracle.build_rings(st, cap=1 << 18, max_rings=1 << 12)
            segs = []
            for r in rings:
                p = r * sc
                p[:, 0] += dx
                p[:, 1] += 0.0
                segs.append(np.concatenate([p[:-1], p[1:]], axis=1))
            segs = np.concatenate(segs)
            assert n_seg is None or len(segs) == n_seg, (name, len(segs))
            assert len(segs) >= 2 * 256, name                        # (512: just below "boxes at all", the rest above)
            names.append(f"{name}@{sc:g}{dx:+g}")
            cmds += [(c[1], c[2], c[3], c[4], c[5], c[6], c[0]) for c in st]
            cmd_off.append(len(cmds))
            scale.append(sc)
            shift.append(dx)
            want.append(segs)
    return (names, np.array(cmd_off, np.uint32), np.array(cmds, dtype=vg.OUTLINE_CMD_DTYPE), np.array(scale), np.array(shift), want)


def test_box_streams_cover_the_branches(box_batch):
    """the generator reaches what it is for: the curves' points cover several chunks, the counts sit on the thresholds"""
    names, cmd_off, _, _, _, want = box_batch
    n = {nm: len(s) for nm, s in zip(names, want)}
    for sc, dx in BOX_SCALES:
        tag = f"@{sc:g}{dx:+g}"
        assert n["quad" + tag] > 256 + 1 and n["cubic" + tag] > 256 + 2
        assert {n["65536" + tag], n["65537" + tag], n["rings(256, 256)" + tag], n["rings(255, 258)" + tag]} == {65536, 65537, 512, 513}


@pytest.mark.parametrize("form", ("into", "prepare"))
def test_command_boxes_against_three_witnesses(oracle, vg, box_batch, form):
    names, cmd_off, cmds, scale, shift, want = box_batch
    c = vg.SdfContext(0)
    try:
        cap = sum(int(np.ceil(s[:, [0, 2]].max()) - np.floor(s[:, [0, 2]].min()) + 8) *
                  int(np.ceil(s[:, [1, 3]].max()) - np.floor(s[:, [1, 3]].min()) + 8) for s in want)
        if form == "into":
            rects, out, ob, ns = c.outlines_render_into(cmd_off, cmds, scale, shift, cap)
        else:
            rects, ob, ns = c.outlines_prepare(cmd_off, cmds, scale, shift)
            out = c.outlines_render()
        assert out is not None and len(out) == ob and ns == sum(len(s) for s in want)
        seg_off, segs = c.outlines_segments()
        # 1. the segments are the oracle's RingBuilder -> scale -> shift, byte for byte
        for g, nm in enumerate(names):
            assert int(rects[g]["has_raster"]) == 1 and int(rects[g]["n_segments"]) == len(want[g]), nm
            assert segs[seg_off[g]:seg_off[g + 1]].tobytes() == want[g].tobytes(), nm
        glyphs = [(want[g], int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])) for g, r in enumerate(rects)]
        batch = vg.make_batch(glyphs)
        # 2. the bitmaps are the oracle's raster of those segments at the device's rects
        ref, _ = oracle.sdf_render_batch(batch, oracle.PRECISE, 8)
        # 3. ... and vgsdf_render_batch's, whose chunk boxes come from the segments themselves
        exact = c.render_batch(batch)
        bad = {}
        for g, nm in enumerate(names):
            a, b = int(batch.out_off[g]), int(batch.out_off[g + 1])
            n_ref, n_exact = int(np.count_nonzero(out[a:b] != ref[a:b])), int(np.count_nonzero(out[a:b] != exact[a:b]))
            if n_ref or n_exact:
                bad[nm] = (n_ref, n_exact)
        assert not bad, bad                           # {glyph: (bytes unlike the oracle's, bytes unlike render_batch's)}
    finally:
        c.close()
