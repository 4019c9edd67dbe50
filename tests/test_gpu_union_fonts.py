"""GPU: union outlines through the façade (vg_manager_set_union_outlines), on the host-tessellation route (upload, union,
launch, download) and on the device front-end's (prepare, vgsdf_outlines_union, render).

Noto Sans Regular, blocks 0-255 and 256-511: with the switch on every glyph's bitmap is the oracle's raster of the RESTATED
union (tests/union_outline_kit.py) of the oracle's segments, its metrics and the PBF framing are those of the switch-off
run, and the stats add up; with the switch off the files are the oracle's (the reference's bytes), before and after a run
with the switch on.  A placed `gvar` instance (tests/gvar_instances_kit.py: an affine image of Fira Sans, whose contours do
not overlap), block 0: every bitmap is the oracle's raster of the restated union of the instance's segments (fontTools' points
at the position); the restatement finds every glyph an identity, so the files are the switch-off files, through the union route."""
import hashlib
import json

import numpy as np
import pytest

import gvar_instances_kit as G
import union_outline_kit as K
from conftest import GOLDEN, NOTO

pytestmark = pytest.mark.gpu
STARTS = (0, 256)


def _varint(b, p):
    v = s = 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, p


def _fields(b):
    """[(field, wire type, value)] of a protobuf message; a length-delimited value as bytes"""
    out, p = [], 0
    while p < len(b):
        key, p = _varint(b, p)
        if key & 7 == 2:
            n, p = _varint(b, p)
            out.append((key >> 3, 2, b[p:p + n]))
            p += n
        else:
            assert key & 7 == 0
            v, p = _varint(b, p)
            out.append((key >> 3, 0, v))
    return out


def glyphs_of(pbf):
    """-> (the file's bytes around the bitmaps: [(field, value) of every glyph but its bitmap], {id: bitmap bytes})"""
    (f, _, stack), = _fields(pbf)
    assert f == 1
    frame, bitmaps = [], {}
    for field, wt, v in _fields(stack):
        if field != 3:
            frame.append((field, v))
            continue
        g = _fields(v)
        gid = [x for fld, _, x in g if fld == 1][0]
        frame.append([(fld, x) for fld, _, x in g if fld != 2])
        for fld, _, x in g:
            if fld == 2:
                bitmaps[gid] = x
    return frame, bitmaps


@pytest.fixture(scope="module")
def hip(vg):
    return vg.Renderer.new_precise(0)


@pytest.fixture(scope="module")
def noto_expected(oracle, noto_oracle):
    """{code point: (oracle bitmap of the restated union, state)} of the two blocks' glyphs with a bitmap; computed once"""
    want = {}
    for cp in range(STARTS[0], STARTS[-1] + 256):
        r = noto_oracle.prepare_glyph(cp)
        if r is None or not r[0].has_bitmap:
            continue
        info, segs = r
        pieces, st = K.union_segments(segs)
        want[cp] = (oracle.sdf_render(pieces, info.x0, info.y0, info.w, info.h).tobytes(), st)
    return want


def _render(vg, hip, fe, union, fid_name="Noto Sans Regular", paths=(NOTO,)):
    m = vg.FontManager(True)
    m.set_device_front_end(fe)
    m.set_union_outlines(union)
    fid = m.add_font_with_name(fid_name, list(paths))
    w = vg.DummyWriter()
    m.render_glyphs(w, hip, fid, list(STARTS))
    return {s: w.files[f"{fid}/{s}-{s + 255}.pbf"] for s in STARTS}, m.union_stats()


@pytest.mark.parametrize("fe", [True, False], ids=["device_front_end", "host_tessellation"])
def test_noto_blocks(vg, oracle, noto_oracle, hip, noto_expected, fe):
    off, stats_off = _render(vg, hip, fe, False)
    on, stats = _render(vg, hip, fe, True)
    again, _ = _render(vg, hip, fe, False)
    assert stats_off == {"seen": 0, "rebuilt": 0, "identity": 0, "over_limit": 0}
    seen = 0
    golden = json.loads((GOLDEN / "pbf_sha256.json").read_text())["noto_regular"]
    for s in STARTS:
        want_off, _, _ = oracle.render_block([noto_oracle], "noto_sans_regular", s, oracle.PRECISE)
        assert off[s] == want_off and again[s] == want_off   # switch off: the reference's bytes, also after a union run ...
        assert hashlib.sha256(off[s]).hexdigest() == golden[str(s)] == hashlib.sha256(again[s]).hexdigest()   # ... the golden SHAs
        frame_on, bm_on = glyphs_of(on[s])
        frame_off, bm_off = glyphs_of(off[s])
        assert frame_on == frame_off                         # ids, metrics, advances, name and range: unchanged
        assert sorted(bm_on) == sorted(bm_off) == sorted(cp for cp in noto_expected if s <= cp < s + 256)
        for cp, bm in bm_on.items():
            assert bm == noto_expected[cp][0], f"U+{cp:04X}"
        seen += len(bm_on)
    # the stats add up: the pass sees every glyph of a submission, those without a bitmap (no segments: identity) included
    states = [st for _, st in noto_expected.values()]
    assert stats["rebuilt"] == states.count(K.STATE_REBUILT) >= 20 and stats["over_limit"] == 0
    assert states.count(K.STATE_IDENTITY) <= stats["identity"] <= states.count(K.STATE_IDENTITY) + 512 - seen
    assert stats["seen"] == stats["rebuilt"] + stats["identity"]
    assert any(on[s] != off[s] for s in STARTS)


@pytest.fixture(scope="module")
def gvar_expected(oracle):
    """{code point: (oracle bitmap of the restated union, state)} of block 0 of the placed instance, from fontTools' points at
    the position and the arithmetic of gvar_instances_kit.yardstick_files (the reference's render_glyph in f64); computed once"""
    import io
    import math

    from fontTools.ttLib import TTFont
    font = G.variable_glyf_fira("shear")
    cbs, widths, _ = G.fonttools_callbacks(font, {"wght": 650})
    scale = 24.0 / TTFont(io.BytesIO(font), lazy=True)["head"].unitsPerEm
    want = {}
    for cp in sorted(c for c in cbs if c < 256):
        adv_units = int(math.floor(widths[cp] + 0.5))
        adv_f = float(adv_units if 0 <= adv_units <= 65535 else 0) * scale * 0.95
        dx = (int(math.floor(adv_f + 0.5)) - adv_f) / 2.0
        rings = oracle.build_rings([(t[0],) + tuple(t[1:]) for t in cbs[cp]])
        if not rings:
            continue
        pts = []
        for r in rings:
            p = r * scale
            p[:, 0] += dx
            pts.append(p)
        allp = np.concatenate(pts)
        minx, miny, maxx, maxy = allp[:, 0].min(), allp[:, 1].min(), allp[:, 0].max(), allp[:, 1].max()
        if maxx <= minx and maxy <= miny:
            continue
        segs = np.concatenate([np.concatenate([p[:-1], p[1:]], axis=1) for p in pts])
        x0, y0 = int(math.floor(minx)) - 3, int(math.floor(miny)) - 3
        x1, y1 = int(math.ceil(maxx)) + 3, int(math.ceil(maxy)) + 3
        pieces, st = K.union_segments(segs)
        want[cp] = (oracle.sdf_render(pieces, x0, y0, x1 - x0, y1 - y0).tobytes(), st)
    return want


@pytest.mark.parametrize("gvar", [False, True], ids=["gvar_on_host", "gvar_on_device"])
def test_a_gvar_instance(vg, hip, gvar_expected, gvar):
    """a placed gvar instance (an affine image of Fira Sans): every bitmap of block 0 with the switch on is the oracle's raster
    of the restated union of the instance's segments; the restatement finds every glyph an identity, the device's stats say the
    same, and so the files are the switch-off files"""
    font = G.variable_glyf_fira("shear")
    files = {}
    for union in (False, True):
        m = vg.FontManager(True)
        m.set_gvar_on_device(gvar)
        m.set_resident_commands(1)
        m.set_union_outlines(union)
        fid = m.add_font_instance("Synth Medium", font, {"wght": 650})
        w = vg.DummyWriter()
        m.render_glyphs(w, hip, fid, [0])
        files[union] = dict(w.files)
        stats = m.union_stats()
    (path, on), = files[True].items()
    frame_on, bm_on = glyphs_of(on)
    frame_off, bm_off = glyphs_of(files[False][path])
    assert frame_on == frame_off and sorted(bm_on) == sorted(gvar_expected) and len(bm_on) >= 50
    for cp, bm in bm_on.items():
        assert bm == gvar_expected[cp][0], f"U+{cp:04X}"
    states = [st for _, st in gvar_expected.values()]
    assert states.count(K.STATE_IDENTITY) == len(states)   # by the restatement: no contour of the instance overlaps another
    assert stats["rebuilt"] == 0 and stats["over_limit"] == 0 and stats["seen"] == stats["identity"] >= len(bm_on)
    assert files[True] == files[False]
