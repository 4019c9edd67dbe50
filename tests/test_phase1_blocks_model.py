"""CPU: tools/model_phase1_blocks.py on the three committed glyph tables -- the model's tile-chunk count stays next to the
counting build's recorded one, its figures are the recorded ones, and its block rule is the kernel's (no GPU)."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import model_phase1_blocks as M  # noqa: E402

# (wave tile-chunks, % of them in a glyph's last chunk, empty blocks of four per tile-chunk): profiles/sweep_diet2_ab.txt
RECORDED = {"noto_regular": (51391, 42.5, 1.72), "fira": (27141, 46.7, 1.94), "noto_all": (199619, 27.4, 1.03)}
COUNTED_NOTO_REGULAR = 51212   # the counting build's wave tile-chunks of one launch (chunks the box test skips are not swept)


def test_the_restated_constants_are_the_kernels():
    csrc = ROOT / "versatiles-glyphs-rs_amd" / "csrc"
    support, kernel = (csrc / "sdf_span_support.h").read_text(), (csrc / "sdf_span_kernel.inc").read_text()
    assert int(re.search(r"constexpr int FCHUNK = (\d+);", support).group(1)) == M.CHUNK
    assert f"constexpr uint32_t GRP = {M.GRP}, NGRP = FCHUNK / GRP;" in kernel
    assert "if (b * 4 < n_groups)" in kernel and "switch ((n_groups + 3) / 4)" in kernel      # both passes: blocks of BLOCK groups
    assert (M.BLOCK, M.BLOCKS) == (4, 8)


def test_real_blocks():
    assert [M.real_blocks(k) for k in (1, 8, 9, 32, 33, 40, 64, 65, 224, 225, 232, 256)] == [1, 1, 1, 1, 2, 2, 2, 3, 7, 8, 8, 8]
    one = M.model([(64, 1)])                   # one wave, one chunk of one record: 7 of its 8 blocks are empty
    assert (one["tile_chunks"], one["last_share"], one["empty_blocks"]) == (1, 1.0, 7.0)
    two = M.model([(65, 256 + 40), (640, 0)])  # two waves x (a full chunk + a chunk of two blocks); a glyph without segments
    assert (two["tile_chunks"], two["last_share"], two["empty_blocks"], two["by_blocks"][2], two["by_blocks"][8]) == (4, 0.5, 3.0, 2, 2)


@pytest.mark.parametrize("workload", list(RECORDED))
def test_recorded_figures(workload):
    m = M.model(M.glyph_table(workload))
    assert (m["tile_chunks"], round(100 * m["last_share"], 1), round(m["empty_blocks"], 2)) == RECORDED[workload]
    assert sum(m["by_blocks"]) == m["tile_chunks"]
    if workload == "noto_regular":              # within 0.5 % of what the counting build counts
        assert 0 <= m["tile_chunks"] - COUNTED_NOTO_REGULAR < 0.005 * COUNTED_NOTO_REGULAR
