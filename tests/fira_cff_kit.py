"""Fira Sans re-encoded as CFF with fontTools: the whole face, or its first 400 glyph ids (listed in front of Fira Sans under one
font id that file draws its code points and Fira the rest).  Shared by the test modules that need a CFF face with known glyphs."""
import pytest


def fira_as_cff(n_glyphs=None):
    """Fira Sans re-encoded as CFF: all of it, or its first n_glyphs glyph ids"""
    pytest.importorskip("fontTools")
    from fontTools.pens.t2CharStringPen import T2CharStringPen
    from fontTools.ttLib import TTFont
    from conftest import FIRA
    from test_cff_outlines import _build
    src = TTFont(FIRA)
    gs = src.getGlyphSet()
    order = src.getGlyphOrder()[:n_glyphs]
    cs = {}
    for g in order:
        pen = T2CharStringPen(gs[g].width, gs)
        gs[g].draw(pen)
        cs[g] = pen.getCharString()
    return _build(order, {cp: g for cp, g in src.getBestCmap().items() if g in cs}, cs, {g: gs[g].width for g in order}, src["head"].unitsPerEm)


@pytest.fixture(scope="module")
def fira_cff_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("cff") / "Fira Sans CFF - Regular.otf"
    path.write_bytes(fira_as_cff())
    return path


@pytest.fixture(scope="module")
def fira_cff_part_file(tmp_path_factory):
    """the first 400 glyph ids only: listed in front of Fira Sans under one font id it draws its code points, Fira the rest"""
    path = tmp_path_factory.mktemp("cff400") / "Fira Sans CFF 400 - Regular.otf"
    path.write_bytes(fira_as_cff(400))
    return path
