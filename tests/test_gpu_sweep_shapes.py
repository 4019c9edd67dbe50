"""GPU: the shapes the span kernel's sweep takes (csrc/sdf_span_kernel.inc), against the oracle (BRUTE), byte for byte, under
both product variants (0: spans, 1: brute force).  The input sets are tests/sweep_shapes_sets.py.

  block counts   phase 1 runs its two passes over blocks of four groups: a full chunk in a straight line, a partial chunk
                 up to its block count, each block's loads issued one block ahead.  One jittered ring per segment count:
                 every block count 1 .. 8, empty groups inside the last real block, the full chunk; windows of one exactly
                 full tile, 255 pixels, and three tiles of which the last is a quarter full
  two shapes     257 .. 808 segments: straight-line and guarded chunks follow each other inside one workgroup
  round counts   phase 2 reads a round's pooled entry one round ahead: waves of one to two rounds, of three to five, and
                 waves past the pool (every lane walks its own list); the counting instance of the margins build
                 (vgsdf_set_variant 61) is the witness that the sets land there

Small on purpose: under 40 glyphs per batch, every bitmap below 1000 pixels."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sweep_shapes_sets as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MARGINS_LIB = ROOT / "versatiles-glyphs-rs_amd" / "build" / "margins" / "libvgsdf.so"


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def run_both(oracle, vg, ctx, glyphs):
    """both product variants equal the oracle's brute force -> the bytes"""
    batch = vg.make_batch(glyphs)
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 4)
    for variant in (0, 1):
        ctx.set_variant(variant)
        got = ctx.render_batch(batch)
        diff = np.flatnonzero(got != want)
        if diff.size:
            g = int(np.searchsorted(batch.out_off, diff[0], side="right")) - 1
            pytest.fail(f"variant {variant}: {diff.size} bytes differ; first: glyph {g} (w {batch.w[g]}, h {batch.h[g]}, "
                        f"{batch.seg_off[g + 1] - batch.seg_off[g]} segments), pixel {int(diff[0] - batch.out_off[g])}, "
                        f"got {got[diff[0]]} want {want[diff[0]]}")
    ctx.set_variant(0)
    return want


def small(glyphs):
    return len(glyphs) < 40 and all(w * h < 1000 for _, _, _, w, h in glyphs)


def test_block_counts_of_one_chunk(oracle, vg, ctx):
    glyphs = S.block_count_glyphs(S.ONE_CHUNK)
    assert small(glyphs) and [len(g[0]) for g in glyphs[:len(S.ONE_CHUNK)]] == list(S.ONE_CHUNK)
    assert {(g[3], g[4]) for g in glyphs} == set(S.WINDOWS)
    run_both(oracle, vg, ctx, glyphs)


def test_straight_line_and_guarded_chunks_in_one_workgroup(oracle, vg, ctx):
    glyphs = S.block_count_glyphs(S.TWO_SHAPES)
    assert small(glyphs) and [len(g[0]) for g in glyphs[:len(S.TWO_SHAPES)]] == list(S.TWO_SHAPES)
    run_both(oracle, vg, ctx, glyphs)


@pytest.mark.parametrize("name", sorted(S.ROUND_SETS))
def test_round_count_sets(oracle, vg, ctx, name):
    glyphs = S.ROUND_SETS[name]()
    assert small(glyphs)
    run_both(oracle, vg, ctx, glyphs)


def test_round_counts_reached(oracle, vg):
    """the counting instance renders the oracle's bytes and counts the rounds the sets were written for"""
    assert MARGINS_LIB.exists(), "the counters need the margins build (make -C versatiles-glyphs-rs_amd margins)"
    cp = subprocess.run([sys.executable, str(ROOT / "tests" / "sweep_shapes_child.py")], cwd=ROOT,
                        env=dict(os.environ, VGSDF_LIB=str(MARGINS_LIB)), capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-3000:]
    doc = json.loads(cp.stdout.strip().splitlines()[-1])
    n = {k: {c: v for c, v in d.items() if c != "bytes"} for k, d in doc.items()}
    print(n)
    for name, gen in S.ROUND_SETS.items():
        want, _ = oracle.sdf_render_batch(vg.make_batch(gen()), oracle.BRUTE, 4)
        assert bytes.fromhex(doc[name]["bytes"]) == want.tobytes(), name
    per_wtc = {k: d["rounds"] / d["wave_tile_chunks"] for k, d in n.items()}
    assert 1.0 < per_wtc["smooth_64gon"] <= 2.0, n
    assert per_wtc["finely_flattened"] > 2.0, n
    assert n["many_ties"]["pool_overflows"] > 0, n
