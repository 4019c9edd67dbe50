"""GPU: the work list's entries (SpanRec, csrc/sdf_kernels.h: the glyph's descriptor travels in every entry) as both planners
write them and both raster kernels read them, bit for bit against the oracle.

One batch holds every kind of entry: span lengths T = 1, 2, 3 and 4, a glyph of several entries, a glyph without pixels (no
entry), glyphs with pixels and no segment, a glyph too wide for the winding histogram (the brute-force class behind n_main),
a glyph whose chunks have boxes (the entry's glyph index), and enough one-span glyphs that the host planner deals the main
class over its eight queues.

  host planner      upload, launch, download (segment arrays: stride 1), variants 0 and 1
  list order off    the same batch with VGSDF_TILE_ORDER=0 in a child process (glyph order, per-XCD remap in the kernel)
  device planner    the same kinds of outline through a front-end submission (outline_plan; segment records: stride 4), once
                    with the raster enqueued behind the plan and once where the plan refuses it (brute-force entries)"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_front_end_regimes import _stream
from test_gpu_span_regimes import CHUNK, TILE, span_count, span_length

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

N_TINY = 70   # one-span glyphs: with them the main class holds >= 64 entries, the host planner's threshold for dealing


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def wavy(n, cx, cy, rx, ry):
    """a closed ring of n segments around (cx, cy), on 1/64 px (exact as the front-end's f32 commands)"""
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    pts = np.stack([cx + rx * np.cos(a) * (1 + 0.1 * np.sin(7 * a)), cy + ry * np.sin(a)], 1)
    return np.round(pts * 64) / 64


TRI = np.array([(1.0, 1.0), (3.0, 1.25), (2.0, 3.0)])


def record_outlines():
    """(name, rings relative to the rect's corner, w, h, T expected in a batch of < 2048 glyphs; 0: brute force, None: no entry)"""
    return [
        ("T4_three_entries", [wavy(40, 12.0, 63.5, 9.0, 58.0)], 24, 127, 4),            # 3048 px: spans of 1024, 1024, 1000
        ("T3_two_px_wide", [np.array([(0.25, 5.0), (1.75, 350.0), (1.5, 690.0), (0.5, 400.0)])], 2, 700, 3),
        ("T2_one_px_wide", [np.array([(0.25, 5.0), (0.75, 300.0), (0.5, 590.0)])], 1, 600, 2),
        ("T2_four_chunks", [wavy(1000, 12.0, 63.5, 9.0, 58.0)], 24, 127, 2),           # boxes in use (> 512 segments)
        ("T1_six_chunks", [wavy(1300, 12.0, 63.5, 9.5, 60.0)], 24, 127, 1),            # boxes in use
        ("T3_wide", [wavy(30, 400.0, 6.0, 390.0, 4.0)], 800, 12, 3),
        ("no_pixels", [TRI], 0, 5, None),
        ("no_segments", [], 3, 3, 4),
        ("no_segments_two_tiles", [], 20, 20, 4),
        ("brute_too_wide", [wavy(60, 750.0, 10.0, 740.0, 6.0)], 1510, 20, 0),
    ] + [(f"tiny{k}", [TRI + (0.25 * (k % 3), 0.0)], 4 + k % 3, 4, 4) for k in range(N_TINY)]


def record_glyphs():
    out = []
    for k, (_, rings, w, h, _) in enumerate(record_outlines()):
        x0, y0 = (k % 5) - 2, 3 - (k % 7)
        segs = np.concatenate([ring(r) for r in rings]) if rings else np.zeros((0, 4))
        out.append((segs + [x0, y0, x0, y0], x0, y0, w, h))
    return out


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records(oracle, vg):
    """the batch and the oracle's bytes, computed once"""
    batch = vg.make_batch(record_glyphs())
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 0)
    return batch, want


def first_difference(batch, got, want):
    diff = np.flatnonzero(got != want)
    if not diff.size:
        return None
    g = int(np.searchsorted(batch.out_off, diff[0], side="right")) - 1
    return f"{diff.size} bytes differ; first: glyph {g} ({record_outlines()[g][0]}), pixel {int(diff[0] - batch.out_off[g])}"


def test_the_batch_holds_the_intended_entries(vg, ctx, records):
    """every kind is present, and the host plan makes the restated number of entries (a wrong T or a lost entry shows)"""
    batch, _ = records
    kinds = record_outlines()
    n = len(kinds)
    assert n < 2048
    want_entries = 0
    for (name, rings, w, h, T), g in zip(kinds, range(n)):
        n_seg = int(batch.seg_off[g + 1] - batch.seg_off[g])
        if T is None:
            assert w * h == 0, name
            continue
        assert (0 if w > 1022 else span_length(w, n_seg, n)) == T, name
        want_entries += span_count(w, h, T)
    assert {k[4] for k in kinds} == {None, 0, 1, 2, 3, 4}
    assert any(k[2] * k[3] > 4 * TILE and k[4] == 4 for k in kinds)                     # several entries of one glyph
    assert sum(1 for g in range(n) if batch.seg_off[g + 1] - batch.seg_off[g] >= 600) >= 2  # chunk boxes in use
    assert any(k[2] * k[3] > 0 and not k[1] for k in kinds)                             # pixels, no segments
    ctx.set_variant(0)
    db = ctx.upload(batch)
    try:
        assert db.stats()["n_tiles"] == want_entries
    finally:
        db.free()


@pytest.mark.parametrize("variant", (0, 1))
def test_host_planned_entries(vg, ctx, records, variant):
    """upload, launch, download: the span kernel over the main class and brute force behind n_main (variant 0), brute force
    over a plain list (variant 1); launched twice, the resident list serves every launch"""
    batch, want = records
    ctx.set_variant(variant)
    db = ctx.upload(batch)
    try:
        for _ in range(2):
            db.launch()
            bad = first_difference(batch, db.download(), want)
            assert bad is None, bad
    finally:
        db.free()
        ctx.set_variant(0)


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, "tests")
from conftest import load_product
import test_gpu_span_records as S
vg = load_product()
c = vg.SdfContext(0)
db = c.upload(vg.make_batch(S.record_glyphs()))
db.launch()
out = db.download()
n = db.stats()["n_tiles"]
db.free()
c.close()
print(json.dumps({"sha": hashlib.sha256(out.tobytes()).hexdigest(), "tiles": n}))
'''


def test_glyph_order_list_in_a_child(records):
    """VGSDF_TILE_ORDER=0 is read per upload: glyph order, no dealing, and the kernel's per-XCD remap of the workgroup index"""
    batch, want = records
    cp = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(os.environ, VGSDF_TILE_ORDER="0"), capture_output=True,
                        text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr[-2000:]
    got = json.loads(cp.stdout.strip().splitlines()[-1])
    assert got["sha"] == hashlib.sha256(want.tobytes()).hexdigest()


def front_end_render(oracle, vg, c, rings_of, capacity=1 << 22):
    """rings_of: per glyph, rings in px -> one front-end submission with room for the bitmaps; checks the bytes against the
    oracle's over the rects and segments the front-end made -> rects"""
    streams = [_stream(r, 1.0) if r else [] for r in rings_of]
    cmds = [(c_[1], c_[2], c_[3], c_[4], c_[5], c_[6], c_[0]) for st in streams for c_ in st]
    cmd_off = np.concatenate([[0], np.cumsum([len(st) for st in streams])]).astype(np.uint32)
    n = len(streams)
    rects, out, ob, ns = c.outlines_render_into(cmd_off, np.array(cmds, dtype=vg.OUTLINE_CMD_DTYPE), np.ones(n), np.zeros(n), capacity)
    if out is None:
        out = c.outlines_render()
    seg_off, segs = c.outlines_segments()
    glyphs = []
    for g in range(n):
        r = rects[g]
        has = int(r["has_raster"])
        glyphs.append((segs[seg_off[g]:seg_off[g + 1]], int(r["x0"]), int(r["y0"]), int(r["w"]) * has, int(r["h"]) * has))
    batch = vg.make_batch(glyphs)
    assert len(out) == ob == batch.out_bytes and ns == len(batch.seg_sx)
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 0)
    diff = np.flatnonzero(out != want)
    if diff.size:
        g = int(np.searchsorted(batch.out_off, diff[0], side="right")) - 1
        pytest.fail(f"{diff.size} bytes differ; first: glyph {g}, pixel {int(diff[0] - batch.out_off[g])}")
    return rects


def front_end_rings(with_brute):
    """the outlines of record_outlines that a command stream can carry (a rect comes from its outline: no rect without one)"""
    rings_of = [rings for name, rings, w, h, T in record_outlines() if rings and w * h and (with_brute or T != 0)]
    return rings_of + [[]]   # and a glyph without commands: no raster, no entry


@pytest.mark.parametrize("with_brute", (False, True), ids=("behind_the_plan", "plan_refuses"))
def test_device_planned_entries(oracle, vg, with_brute):
    """outline_plan writes the entries; the raster enqueued behind it reads them with the plan's verdict.  First case: twice on
    one context, so that the second submission meets capacities the first one sized and its plan says "ok".  Second case: the
    verdict is "not ok" whatever the capacities, because the list holds brute-force entries, and the host launches both
    kernels afterwards"""
    c = vg.SdfContext(0)
    try:
        rects = front_end_render(oracle, vg, c, front_end_rings(with_brute))
        if not with_brute:
            rects = front_end_render(oracle, vg, c, front_end_rings(with_brute))
        widths = [int(r["w"]) for r in rects if int(r["has_raster"])]
        assert (max(widths) > 1022) == with_brute
        n_seg = np.diff(c.outlines_segments()[0])
        assert int(n_seg.max()) > 2 * CHUNK          # chunk boxes in use: the entry's glyph index
    finally:
        c.close()
