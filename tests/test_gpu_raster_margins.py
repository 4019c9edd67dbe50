"""GPU: the numerical margins of the default raster kernel under directed inputs.

Product: every set of tests/raster_margin_sets.py through variants 0 (bounded groups over spans) and 1 (brute force), both
equal to the oracle byte for byte.  These guard the product whether or not the margins build exists.

Margins build (`make margins`, csrc/sdf_margin_kernels.hip): ONE child process renders every set with the `base`
instance (today's margins: zero differing bytes on every set, old and new), with the counting instance (which branches
a set reaches) and with every weakened instance, each of which has one margin switched off and MUST give wrong bytes on
the set written to catch it:

    instance       margin switched off                               caught by set
    a_dl0          dl := 0, no `8 e <= f1`: byte from the f32 bin     near_boundary
                                                                      (near_subulp: the same below the f64 resolution)
    b_e0           e := 0 (h(F) and e64) in decide, ub2, Tk           near_M4000
    c_tk_f1        Tk := f1: only the filter's argmin is exact        argmin_swap
    d_rg0          r_g := 0 in the candidate rule                     cand_long_in_group
    e_sat3         SAT 6.2 -> 3.0 in phase 1                          cand_sat_far
    f_far20        far 35.9 -> 20                                     cand_sat_far
    g_sane         `sane` always true (filter trusted at M >= 10^6)   guard_huge
    h_bounded      `bounded` always true (group bounds at M >= 4096)  none: cannot change a byte (DESIGN.md §4.1:
                                                                      the pad 0.01 + 1e-5 M grows with M); asserted
                                                                      equal to the oracle on every set
    i_box_r0       chunk-box skip with R := 0                         box_reach
    j_box_band     chunk-box skip without the row-band condition      box_band
    k_e64_0        e64 := 0 alone                                     none: cannot change a byte for int32 rect origins
    k_mabs0_0      mabs0 := 0 alone                                   (the slack 64 - 47 of h(F) covers the
                                                                      reference's own error); asserted equal to the oracle
                                                                      on every set, abs_position (origins 2^23, 2^24) included
    l_infl_pad     INFL, pad, 1.004 := 1, 0, 1                        cand_equality

The instances at 1/2, 1/4, 1/8 of e, dl and r_g are recorded (profiles/raster_margin_kills.txt), not asserted.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import raster_margin_sets as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MARGINS_LIB = ROOT / "versatiles-glyphs-rs_amd" / "build" / "margins" / "libvgsdf.so"

DIRECTED = {"a_dl0": "near_boundary", "b_e0": "near_M4000", "c_tk_f1": "argmin_swap", "d_rg0": "cand_long_in_group",
            "e_sat3": "cand_sat_far", "f_far20": "cand_sat_far", "g_sane": "guard_huge", "i_box_r0": "box_reach",
            "j_box_band": "box_band", "l_infl_pad": "cand_equality"}
NEUTRAL = ("h_bounded", "k_e64_0", "k_mabs0_0")  # DESIGN.md §4.1 argues they cannot change a byte and names the quantities as removable


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(S.new_sets()))
def test_product_variants_equal_the_oracle(oracle, vg, ctx, name):
    batch = vg.make_batch(S.new_sets()[name].glyphs)
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE, 4)
    try:
        for variant in (0, 1):
            ctx.set_variant(variant)
            diff = np.flatnonzero(ctx.render_batch(batch) != want)
            assert diff.size == 0, f"{name}, variant {variant}: {diff.size} bytes differ, first at {diff[:5]}"
    finally:
        ctx.set_variant(0)


@pytest.fixture(scope="module")
def margins():
    """the matrix of the margins build: one child process, ended at its first error"""
    if not MARGINS_LIB.exists():
        pytest.fail(f"{MARGINS_LIB} is missing: build it with `make -C versatiles-glyphs-rs_amd margins` (the default `make` "
                    "target, i.e. build(), does)")
    env = dict(os.environ, VGSDF_LIB=str(MARGINS_LIB))
    cp = subprocess.run([sys.executable, str(ROOT / "tests" / "raster_margin_child.py")], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=240)
    assert cp.returncode == 0, cp.stderr[-3000:]
    return json.loads(cp.stdout.strip().splitlines()[-1])


def test_base_instance_equals_the_oracle_on_every_set(margins):
    assert set(S.new_sets()) < set(margins["pixels"]) and any(n.startswith("old_") for n in margins["pixels"])
    for inst in ("product_0", "base", "count"):
        wrong = {n: d for n, d in margins["diff"][inst].items() if d}
        assert not wrong, (inst, wrong)


@pytest.mark.parametrize("inst", sorted(DIRECTED))
def test_weakened_instance_is_caught_by_its_directed_set(margins, inst):
    row = margins["diff"][inst]
    print(inst, {n: d for n, d in row.items() if d})
    assert row[DIRECTED[inst]] > 0, f"{inst} survives {DIRECTED[inst]}; caught by: { {n: d for n, d in row.items() if d} }"


@pytest.mark.parametrize("inst", NEUTRAL)
def test_instance_argued_neutral_changes_no_byte(margins, inst):
    wrong = {n: d for n, d in margins["diff"][inst].items() if d}
    assert not wrong, (inst, wrong)


def test_every_weakened_instance_is_listed():
    from raster_margin_child import WEAKENED
    assert sorted(WEAKENED) == sorted(list(DIRECTED) + list(NEUTRAL))


def test_counters_show_the_intended_branches(margins):
    c = margins["counters"]
    sets = S.new_sets()
    for name, s in sets.items():
        assert c[name]["wave_tile_chunks"] > 0 or (s.M or 0) >= 1.0e6, name
        if s.near and name != "near_M1e6hi":
            assert c[name]["undecided_lanes"] > 0, (name, c[name])
    # M >= 10^6: the filter is off (every segment of the chunk exactly, for every pixel): no lane is ever "undecided"
    assert c["near_M1e6hi"]["undecided_lanes"] == 0 and c["near_M1e6hi"]["wave_tile_chunks"] == 0, c["near_M1e6hi"]
    for name in ("lanes_1", "lanes_2"):      # 1 .. VG_POOL_MAX undecided lanes: the wave evaluates them together
        assert c[name]["waves_pooled_exact"] > 0, (name, c[name])
    for name in ("lanes_3", "lanes_row"):    # more: every lane for itself
        assert c[name]["waves_per_lane_exact"] > 0, (name, c[name])
    assert any(c[n]["pool_overflows"] > 0 for n, s in sets.items() if s.M is not None and 4096 <= s.M < 1.0e6), \
        {n: c[n]["pool_overflows"] for n in c}
