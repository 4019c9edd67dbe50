"""CPU: tools/model_stage_filters.py, the numpy restatement of the stage's f32 decision ("The stage's
integers"), on Fira Sans and on the directed sets of tests/stage_filter_sets.py.

With the margin in place no decided bracket may differ from first_ge's; with the margin at 0 the set written to catch the
weakened instance of `make margins` must hold a wrong bracket, or the GPU test that expects wrong bytes cannot pass.  The
model also carries the column filter that was built, measured and not kept: it must never differ either."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import model_stage_filters as M  # noqa: E402
import stage_filter_sets as S  # noqa: E402


def test_fira_sans_has_no_differing_decision():
    m = M.batch_model(M.font_glyphs("fira"))
    M.report("fira", m)
    assert m["segs"] > 100000 and m["pairs"] > 10000
    assert m["row_bad"] == 0 and m["xc_bad"] == 0
    # the f64 paths stay rare on a real font: well under 1 % of the lanes and of the pairs
    assert m["row_und"] < 0.01 * m["segs"] and m["xc_und"] < 0.01 * m["pairs"]


@pytest.fixture(scope="module")
def set_models():
    return {name: M.batch_model(glyphs) for name, glyphs in S.sets().items()}


def test_margined_decisions_never_differ_on_the_directed_sets(set_models):
    wrong = {n: (m["row_bad"], m["xc_bad"]) for n, m in set_models.items() if m["row_bad"] or m["xc_bad"]}
    assert not wrong, wrong


def test_unmargined_brackets_differ_on_far_row(set_models):
    assert set_models["far_row"]["row_bad0"] > 0


def test_sets_reach_the_paths_they_are_named_for(set_models):
    assert set_models["far_insane"]["row_und"] == set_models["far_insane"]["segs"]
    assert set_models["row_edge"]["row_und"] > 0 and set_models["far_row"]["row_und"] > 0
    for g in S.walk():                                                   # more pairs in the one wave than the pool's 256
        assert M.glyph_model(*g)["pairs"] > 256 and len(g[0]) == 64
