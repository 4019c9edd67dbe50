"""CPU: tools/model_wave_shares.py on the three font batches -- the restated planner reproduces the recorded work list of
Noto Sans Regular, and the kernel's rotation hash meets the conditions it was chosen under (no GPU: the batches come from the
product's host stage)."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import model_wave_shares as M  # noqa: E402


def test_the_restated_hash_is_the_kernels():
    src = (ROOT / "versatiles-glyphs-rs_amd" / "csrc" / "sdf_span_support.h").read_text()
    assert int(re.search(r"WAVE_ROT_MUL = (0x[0-9A-Fa-f]+)u;", src).group(1), 16) == M.WAVE_ROT_MUL
    assert "return (b * WAVE_ROT_MUL) >> 30;" in src
    assert [M.wave_rot(b) for b in (0, 1, 8, 13, 3022)] == [(b * M.WAVE_ROT_MUL % 2 ** 32) >> 30 for b in (0, 1, 8, 13, 3022)]


@pytest.mark.parametrize("workload", ("noto_regular", "fira", "noto_all"))
def test_rotated_shares(workload):
    m = M.model(*M.batch_shapes(workload))
    today, rotated = m["today"].sum(axis=0), m["rotated"].sum(axis=0)
    assert today.sum() == rotated.sum()                       # the same sweeps, placed differently
    if workload == "noto_regular":                             # the recorded list: 3023 workgroups, its chain histogram, the shares
        assert m["workgroups"] == 3023
        vals, cnt = np.unique(m["chain"], return_counts=True)
        assert [(int(v), int(c)) for v, c in zip(vals, cnt)][-5:] == [(12, 213), (14, 12), (15, 76), (16, 28), (18, 3)]
        assert today.tolist() == [15055, 13578, 12234, 10524]
    assert M.spread(today) > 1.1
    assert M.spread(rotated) <= M.LIMIT_ALL
    assert M.block_spread(m["rotated"]) <= M.LIMIT_BLOCK
