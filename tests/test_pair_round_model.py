"""CPU: tools/model_pair_rounds.py on the first glyphs of Noto Sans Regular -- its figures stay next to what the counting
instance of the margins build counted on the same glyphs on an MI355X, its own recorded figures are reproduced, and its
constants are the kernel's (no GPU)."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import model_pair_rounds as M  # noqa: E402

GLYPHS = 300
# the counting instance on the first 300 glyphs of the headline batch, one launch (profiles/pair_rounds_ab.txt)
COUNTED = {"wave_tile_chunks": 4959, "pairs": 511555, "rounds": 9901, "pool_overflows": 281, "half_rounds": 1786,
           "left_after_phase1": 956}
# the model on the same glyphs (the whole batch: 51 391 sweeps, 5 257 912 pairs, 2955 above QCAP with 888 732 pairs, 9043 without a pair)
RECORDED = {"sweeps": 5031, "pairs": 512964, "rounds": 9917, "over": 284, "over_pairs": 84217, "no_pair": 1028,
            "tails": {"0": 1028, "1-16": 930, "17-32": 850, "33-64": 1939}}


@pytest.fixture(scope="module")
def fig():
    n, sweeps = M.sweeps_of("noto_regular", GLYPHS)
    assert n == GLYPHS
    return M.model(sweeps)


def test_the_restated_constants_are_the_kernels():
    csrc = ROOT / "versatiles-glyphs-rs_amd" / "csrc"
    support, kernel = (csrc / "sdf_span_support.h").read_text(), (csrc / "sdf_span_kernel.inc").read_text()
    assert int(re.search(r"constexpr int FCHUNK = (\d+);", support).group(1)) == M.CH
    assert f"constexpr uint32_t GRP = {M.GRP}, NGRP = FCHUNK / GRP;" in kernel
    assert int(re.search(r"constexpr uint32_t QCAP = (\d+);", kernel).group(1)) == M.QCAP


def test_recorded_figures(fig):
    assert {k: fig[k] for k in RECORDED} == RECORDED
    assert sum(fig["tails"].values()) == fig["sweeps"] - fig["over"]


def test_within_two_percent_of_the_counting_build(fig):
    def near(model, counted):
        return abs(model - counted) <= 0.02 * counted
    # the model does not skip chunks by their box: it sweeps a little more, and every sweep it has too many is one without a pair
    extra = fig["sweeps"] - COUNTED["wave_tile_chunks"]
    assert 0 <= extra and near(fig["sweeps"], COUNTED["wave_tile_chunks"])
    assert near(fig["pairs"], COUNTED["pairs"]) and near(fig["rounds"], COUNTED["rounds"])
    assert near(fig["over"], COUNTED["pool_overflows"])
    assert near(fig["tails"]["1-16"] + fig["tails"]["17-32"], COUNTED["half_rounds"])
    assert near(fig["no_pair"] - extra, COUNTED["left_after_phase1"])


def test_window_costs_and_policies():
    assert M.window_costs(0, True, True) == 0
    assert [M.window_costs(n, False, False) for n in (1, 32, 33, 64, 65, 256)] == [M.ROUND * k for k in (1, 1, 1, 1, 2, 4)]
    assert M.window_costs(32, True, False) == M.HALF_ROUND and M.window_costs(33, True, False) == M.ROUND
    assert M.window_costs(96, True, False) == M.ROUND + M.HALF_ROUND
    assert M.window_costs(16, True, True) == M.QUARTER_ROUND and M.window_costs(17, True, True) == M.HALF_ROUND
    f = M.model(np.array([[0, 0], [30, 1], [300, 9], [64, 2]]))
    assert (f["sweeps"], f["pairs"], f["over"], f["no_pair"], f["tails"]) == (4, 394, 1, 1, {"0": 1, "1-16": 0, "17-32": 1, "33-64": 1})
    v = f["valu_per_sweep"]
    assert v["today"] == (M.ROUND + 9 * M.WALK_GROUP + M.ROUND) / 4
    assert v["passes"] == (M.ROUND + 5 * M.ROUND + M.ROUND) / 4              # 300 = a window of 256 and one of 44
    assert v["half"] == (M.HALF_ROUND + 5 * M.ROUND + M.ROUND) / 4
    assert v["half, walk kept"] == (M.HALF_ROUND + 9 * M.WALK_GROUP + M.ROUND) / 4
