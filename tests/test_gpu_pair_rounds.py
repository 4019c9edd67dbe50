"""GPU: phase 2's pair rounds of the span kernel (csrc/sdf_span_kernel.inc) at the totals where a sweep changes its shape --
the half round for a last round of at most 32 entries, the per-lane walk of a sweep of more than QCAP pairs (the totals past
QCAP are the windows' edges of a sweep pooled in passes, which was measured and not kept), the leave behind phase 1 of a wave
without a pair -- against the oracle (BRUTE), byte for byte, under both product variants (0: spans, 1: brute force)
and under the counting instance of the margins build (vgsdf_set_variant 61), whose counters are the witness that a set's
total is the arithmetic's.  The sets are tests/pair_round_sets.py (tests/test_pair_round_sets_host.py checks them on the CPU).

`pairs`, `rounds` and `pool_overflows` count a sweep's INPUT (total, (total + 63) / 64, total > QCAP), not how it was
processed: they hold for any library that renders these sets.  `half_rounds` and `left_after_phase1` count the processing
and have tests of their own."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pair_round_sets as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MARGINS_LIB = ROOT / "versatiles-glyphs-rs_amd" / "build" / "margins" / "libvgsdf.so"


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(oracle, vg):
    """the oracle's bytes of every set, computed once"""
    return {name: oracle.sdf_render_batch(vg.make_batch(gen()), oracle.BRUTE, 4)[0] for name, gen in S.SETS.items()}


@pytest.fixture(scope="module")
def counted():
    """every set through the counting instance, in one child process"""
    assert MARGINS_LIB.exists(), "the counters need the margins build (make -C versatiles-glyphs-rs_amd margins)"
    cp = subprocess.run([sys.executable, str(ROOT / "tests" / "pair_round_child.py")], cwd=ROOT,
                        env=dict(os.environ, VGSDF_LIB=str(MARGINS_LIB)), capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-3000:]
    doc = json.loads(cp.stdout.strip().splitlines()[-1])
    print({k: {c: v for c, v in d.items() if c != "bytes"} for k, d in doc.items()})
    return doc


@pytest.mark.parametrize("name", sorted(S.SETS))
def test_bytes(vg, ctx, want, name):
    batch = vg.make_batch(S.SETS[name]())
    for variant in (0, 1):
        ctx.set_variant(variant)
        got = ctx.render_batch(batch)
        diff = np.flatnonzero(got != want[name])
        if diff.size:
            ctx.set_variant(0)
            g = int(np.searchsorted(batch.out_off, diff[0], side="right")) - 1
            pytest.fail(f"variant {variant}: {diff.size} bytes differ; first: glyph {g} (w {batch.w[g]}, h {batch.h[g]}), "
                        f"pixel {int(diff[0] - batch.out_off[g])}, got {got[diff[0]]} want {want[name][diff[0]]}")
    ctx.set_variant(0)


@pytest.mark.parametrize("name", sorted(S.SETS))
def test_counting_instance_bytes(counted, want, name):
    assert bytes.fromhex(counted[name]["bytes"]) == want[name].tobytes()


@pytest.mark.parametrize("name", sorted(S.FAR_SETS))
def test_totals_are_the_arithmetics(counted, name):
    got = {k: counted[name][k] for k in ("pairs", "rounds", "wave_tile_chunks", "pool_overflows")}
    assert got == S.far_counters(S.FAR_SETS[name]())


def test_near_sets_totals(counted):
    """bounded regime: one group is a candidate of every owning lane (its own anchor sets the bound); two chunks x the three waves of a 12 x 12 window"""
    n = counted["winner_halves"]
    assert (n["pairs"], n["rounds"], n["wave_tile_chunks"], n["pool_overflows"]) == (30, 1, 1, 0)
    for name in ("no_pair_behind", "no_pair_first"):
        assert counted[name]["wave_tile_chunks"] == 2 * 3 and counted[name]["pairs"] > 0, name
        assert counted[name]["rounds"] >= 1


def tail(total):
    return (total - 1) % 64 + 1


def test_half_rounds_taken(counted):
    """how the sweeps were processed: a half round wherever a pooled sweep (total <= QCAP) ends in 1 .. 32 entries"""
    for name in sorted(S.FAR_SETS):
        totals = [L * g for segs, _, _, w, h in S.FAR_SETS[name]() for g in S.n_groups(len(segs)) for L in S.owning_lanes(w, h)]
        assert counted[name]["half_rounds"] == sum(t <= S.QCAP and tail(t) <= 32 for t in totals), name
    assert counted["winner_halves"]["half_rounds"] == 1 and counted["short_last_group_near"]["half_rounds"] == 3
    assert counted["total_0032"]["half_rounds"] == 1 and counted["total_0033"]["half_rounds"] == 0
    assert counted["total_0096"]["half_rounds"] == 1 and counted["total_0258"]["half_rounds"] == 0


def test_left_after_phase1(counted):
    """the chunk out of every pixel's reach: each of the window's three waves leaves its sweep behind phase 1"""
    for name in ("no_pair_behind", "no_pair_first"):
        assert counted[name]["left_after_phase1"] >= 3, name
    assert all(counted[name]["left_after_phase1"] == 0 for name in S.FAR_SETS)
