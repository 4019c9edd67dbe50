"""GPU: the stage of the default raster kernel ("The stage's integers") under directed inputs.

The stage takes a segment's bracket of sample rows from the f32 record where both end points lie farther than E_row from every
row centre, and from first_ge in f64 otherwise; a crossing's column always comes from the f64 crossing and first_ge.  Every set
of tests/stage_filter_sets.py goes through product variants 0 (bounded groups over spans) and 1 (brute force) and must equal
the oracle byte for byte, in its PRECISE and in its BRUTE mode:

    row_edge    end points at a row centre +- 2^-j (j = 10 .. 52) and on it, both ends, up and down: the half-open rule
    col_edge    vertical and 3-4-5 edges crossing at a column centre +- 2^-j and on it; column 0 and the cell w
    flat        |dy| = 2^-20 .. 2^-40 across one row
    far_row     row_edge with the edges extended to M = 4000
    far_col     col_edge at M = 4000, and 3-4-5 edges at M = 9e5
    far_insane  just above M = 10^6: no f32 decision at all
    walk        64 near-vertical segments over 35 rows each: more pairs than the pool holds, every thread walks its rows
    partial     last chunks of 1, 7, 8 and 9 records, the long member of the last group away from its anchor
    wide_rows   w = 3, 255, 256, 257 over spans of 1 .. 4 tiles
    fuzz        300 random small glyphs

Margins build (`make margins`): one child process renders every set with `base` (must equal the oracle), with the counting
instance, and with the weakened instance VG_M_ROW_E := 0, which must give wrong bytes on far_row.
tools/model_stage_filters.py predicts that on the CPU (tests/test_stage_filter_model.py).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import stage_filter_sets as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MARGINS_LIB = ROOT / "versatiles-glyphs-rs_amd" / "build" / "margins" / "libvgsdf.so"


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def references(oracle, vg):
    """per set: the batch and the oracle's bytes, rendered once (BRUTE and PRECISE agree, or the set itself is no test)"""
    out = {}
    for name, glyphs in S.sets().items():
        batch = vg.make_batch(glyphs)
        brute, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 8)
        precise, _ = oracle.sdf_render_batch(batch, oracle.PRECISE, 8)
        out[name] = (batch, brute, precise)
    return out


@pytest.mark.parametrize("name", sorted(S.sets()))
def test_product_variants_equal_the_oracle(references, ctx, name):
    batch, brute, precise = references[name]
    try:
        for variant in (0, 1):
            ctx.set_variant(variant)
            got = ctx.render_batch(batch)
            for mode, want in (("BRUTE", brute), ("PRECISE", precise)):
                diff = np.flatnonzero(got != want)
                assert diff.size == 0, f"{name}, variant {variant} against {mode}: {diff.size} bytes differ, first at {diff[:5]}"
    finally:
        ctx.set_variant(0)


@pytest.fixture(scope="module")
def margins():
    """the stage's instances of the margins build: one child process, ended at its first error"""
    if not MARGINS_LIB.exists():
        pytest.fail(f"{MARGINS_LIB} is missing: build it with `make -C versatiles-glyphs-rs_amd margins` (the default `make` "
                    "target, i.e. build(), does)")
    env = dict(os.environ, VGSDF_LIB=str(MARGINS_LIB))
    cp = subprocess.run([sys.executable, str(ROOT / "tests" / "stage_filter_child.py")], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=240)
    assert cp.returncode == 0, cp.stderr[-3000:]
    return json.loads(cp.stdout.strip().splitlines()[-1])


def test_base_instance_equals_the_oracle_on_every_set(margins):
    assert set(S.sets()) == set(margins["pixels"])
    for inst in ("product_0", "base", "count"):
        wrong = {n: d for n, d in margins["diff"][inst].items() if d}
        assert not wrong, (inst, wrong)


def test_row_margin_switched_off_is_caught_by_far_row(margins):
    row = margins["diff"]["m_row_e0"]
    print({n: d for n, d in row.items() if d})
    assert row["far_row"] > 0, f"VG_M_ROW_E := 0 survives far_row; caught by: { {n: d for n, d in row.items() if d} }"


def test_counter_shows_the_fallback_and_its_absence(margins):
    c = margins["counters"]
    print(c)
    for name in ("row_edge", "far_row", "far_insane", "flat"):
        assert c[name]["row_fallback_waves"] > 0, (name, c[name])
    # outlines whose end points lie well away from every row centre never take the f64 brackets
    assert c["walk"]["row_fallback_waves"] == 0 and c["wide_rows"]["row_fallback_waves"] == 0
