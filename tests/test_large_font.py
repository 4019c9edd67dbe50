"""A font of CJK scale through the whole pipeline: 20 000 glyphs (random closed contours of lines and quadratics) on the code
points U+4E00.., synthesised with fontTools (the reference's testdata lacks its Noto Sans JP / KR / SC files:
.MISSING_LARGE_BLOBS).  Four groups of >= 5000 glyphs in flight two at a time, capacities that grow from one group to the
next, block files far from the first ones.  Expected bytes: the oracle's.  CPU: dummy raster; GPU: HIP raster through both
dispatchers and through three device lanes."""
import io

import numpy as np
import pytest

pytest.importorskip("fontTools")
from fontTools.fontBuilder import FontBuilder  # noqa: E402
from fontTools.pens.ttGlyphPen import TTGlyphPen  # noqa: E402

N_GLYPHS = 20000
FIRST_CP = 0x4E00


@pytest.fixture(scope="module")
def big_font():
    rng = np.random.default_rng(20261004)
    order, cmap, glyphs, metrics = [".notdef"], {}, {".notdef": TTGlyphPen(None).glyph()}, {".notdef": (500, 0)}
    for i in range(N_GLYPHS):
        name = f"g{i}"
        pen = TTGlyphPen(None)
        for _ in range(int(rng.integers(1, 4))):
            cx, cy, r = rng.integers(150, 850), rng.integers(0, 700), rng.integers(40, 300)
            k = int(rng.integers(3, 9))
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            pts = [(int(cx + r * np.cos(a)), int(cy + r * np.sin(a))) for a in ang]
            pen.moveTo(pts[0])
            for j in range(1, k):
                if rng.random() < 0.6:
                    mid = ((pts[j - 1][0] + pts[j][0]) // 2 + int(rng.integers(-60, 60)), (pts[j - 1][1] + pts[j][1]) // 2 + int(rng.integers(-60, 60)))
                    pen.qCurveTo(mid, pts[j])
                else:
                    pen.lineTo(pts[j])
            pen.closePath()
        glyphs[name] = pen.glyph()
        order.append(name)
        cmap[FIRST_CP + i] = name
        metrics[name] = (int(rng.integers(400, 1100)), 0)
    fb = FontBuilder(1000, isTTF=True)
    fb.setupGlyphOrder(order)
    fb.setupCharacterMap(cmap)
    fb.setupGlyf(glyphs)
    fb.setupHorizontalMetrics(metrics)
    fb.setupHorizontalHeader(ascent=900, descent=-100)
    fb.setupNameTable({"familyName": "Big Synthetic", "styleName": "Regular"})
    fb.setupOS2()
    fb.setupPost()
    buf = io.BytesIO()
    fb.save(buf)
    return buf.getvalue()


def _oracle_files(oracle, data, fid, mode):
    font = oracle.Font(data)
    return {f"{fid}/{b * 256}-{b * 256 + 255}.pbf": oracle.render_block([font], fid, b * 256, mode)[0] for b in range(256)}


@pytest.fixture(scope="module")
def precise_files(oracle, big_font):
    """the oracle's PRECISE files of the font (its id is "big_synthetic_regular"; computed once for the module)"""
    return _oracle_files(oracle, big_font, "big_synthetic_regular", oracle.PRECISE)


# Groups of exactly these many glyphs: the device front-end's plan has instances and run lengths that change at 4096 /
# 4097 and 8192 / 8193 glyphs, and above 8192 places every glyph twice (outline_plan<8, false>); 4352 and 8448 sit one
# block past the edges, 20 000 is the whole font in one submission.
GROUP_GLYPHS = (4096, 4352, 8192, 8448, N_GLYPHS)


def _groups(counts, bpb):
    """glyph counts of the dispatcher's groups with set_threads(_, bpb): one task per block of the font, in block order
    (render_glyphs), cut into runs of bpb tasks (run_tasks / run_tasks_device_front_end)"""
    return [int(counts[i:i + bpb].sum()) for i in range(0, len(counts), bpb)]


def _blocks_per_batch_for(counts, glyphs):
    """the smallest blocks_per_batch whose largest group holds exactly `glyphs` glyphs"""
    for bpb in range(1, len(counts) + 1):
        if max(_groups(counts, bpb)) == glyphs:
            return bpb
    raise AssertionError(f"no blocks_per_batch gives a group of {glyphs} glyphs")


def test_large_font_dummy(vg, oracle, big_font):
    m = vg.FontManager(True)
    fid = m.add_font_data("Big Synthetic Regular", big_font)
    assert int(m.block_counts(fid).sum()) == N_GLYPHS
    w = vg.DummyWriter()
    m.render_glyphs(w, vg.Renderer.new_dummy())
    assert w.files == _oracle_files(oracle, big_font, fid, oracle.DUMMY)


def test_group_counters_with_blocks_per_batch(vg, oracle, big_font):
    """fe_groups / fe_max_group_glyphs of the timings report the dispatcher's groups (here the host dispatcher's, whose
    groups of set_threads(_, n) are the device front-end's): the blocks_per_batch values of the GPU test below really
    give groups of 4096, 4352, 8192, 8448 and 20 000 glyphs"""
    m = vg.FontManager(True)
    fid = m.add_font_data("Big Synthetic Regular", big_font)
    counts = m.block_counts(fid)
    assert list(np.flatnonzero(counts)) == list(range(0x4E, 0x9D)) and int(counts[0x9C]) == 32
    want = _oracle_files(oracle, big_font, fid, oracle.DUMMY)
    r = vg.Renderer.new_dummy()
    bpbs = [_blocks_per_batch_for(counts, n) for n in GROUP_GLYPHS]
    assert bpbs == [16, 17, 32, 33, 157]
    for bpb, n in zip(bpbs, GROUP_GLYPHS):
        m.set_threads(0, bpb)
        w = vg.DummyWriter()
        m.render_glyphs(w, r)
        t = m.timings()
        sizes = [s for s in _groups(counts, bpb) if s]
        assert (t["fe_groups"], t["fe_max_group_glyphs"], t["glyphs"]) == (len(sizes), n, N_GLYPHS), (bpb, t)
        assert w.files == want, bpb


@pytest.mark.gpu
def test_large_font_on_the_gpu(vg, big_font, precise_files):
    m = vg.FontManager(True)
    fid = m.add_font_data("Big Synthetic Regular", big_font)
    want = precise_files
    assert set(want) == {f"{fid}/{b * 256}-{b * 256 + 255}.pbf" for b in range(256)}
    r = vg.Renderer.new_precise(0)
    for fe in (True, False):
        m.set_device_front_end(fe)
        w = vg.DummyWriter()
        m.render_glyphs(w, r)
        bad = [n for n in want if w.files[n] != want[n]]
        assert not bad, (fe, len(bad), bad[:3])
        assert m.timings()["glyphs"] == N_GLYPHS
    m.set_device_front_end(True)
    w = vg.DummyWriter()
    m.render_glyphs(w, vg.Renderer.new_multi([0, 0, 0]))
    assert w.files == want
    # a second font in the same manager: groups now span fonts
    from conftest import FIRA
    m.add_font_with_name("Fira Sans Regular", [FIRA])
    w = vg.DummyWriter()
    m.render_glyphs(w, r)
    assert all(w.files[n] == want[n] for n in want) and len(w.files) == 512


@pytest.mark.gpu
@pytest.mark.parametrize("glyphs", GROUP_GLYPHS)
def test_front_end_groups_of_plan_edge_sizes(vg, big_font, precise_files, glyphs):
    """the device front-end with groups of exactly `glyphs` glyphs (set_threads(_, blocks_per_batch)), blocks assembled in
    place and encoded afterwards, `glyf` decoded on the device and recorded by the host: every file is the oracle's, and the
    timings show that the intended group was submitted"""
    m = vg.FontManager(True)
    fid = m.add_font_data("Big Synthetic Regular", big_font)
    counts = m.block_counts(fid)
    bpb = _blocks_per_batch_for(counts, glyphs)
    sizes = [s for s in _groups(counts, bpb) if s]
    m.set_threads(0, bpb)
    m.set_device_front_end(True)
    r = vg.Renderer.new_precise(0)
    for in_place in (True, False):
        for on_device in (True, False):
            m.set_in_place_pbf(in_place)
            m.set_glyf_on_device(on_device)
            w = vg.DummyWriter()
            m.render_glyphs(w, r)
            t = m.timings()
            key = (glyphs, bpb, in_place, on_device)
            assert (t["fe_groups"], t["fe_max_group_glyphs"], t["glyphs"]) == (len(sizes), glyphs, N_GLYPHS), (key, t)
            assert (t["glyf_groups"], t["glyf_fallbacks"]) == ((len(sizes) if on_device else 0), 0), (key, t)
            bad = [n for n in precise_files if w.files[n] != precise_files[n]]
            assert not bad and len(w.files) == 256, (key, len(bad), bad[:3])
