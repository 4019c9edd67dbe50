"""GPU: adversarial and synthetic inputs straight at the C ABI (vgsdf_render_batch), both
kernel variants (0 = filtered, 1 = brute force) against the oracle.  Covers what the font
fixtures do not: ties, degenerate segments, winding +-2, samples exactly on vertices / rows,
queue overflow, multi-chunk segment lists, wide / thin rects, big coordinates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    yield c
    c.close()


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def run_both(oracle, vg, ctx, glyphs, mode=None):
    """glyphs: [(segs, x0, y0, w, h)] -> asserts both variants equal the oracle"""
    batch = vg.make_batch(glyphs)
    want, _ = oracle.sdf_render_batch(batch, oracle.BRUTE if mode is None else mode, 4)
    for variant in (0, 1):  # default (bounded groups over spans) and brute force: all the product build exports
        ctx.set_variant(variant)
        got = ctx.render_batch(batch)
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, f"variant {variant}: {diff.size} bytes differ, first at {diff[:5]}"
    ctx.set_variant(0)
    return batch, want


def random_polys(rng, n_glyphs, n_rings, n_pts, size, jitter=0.35):
    out = []
    for _ in range(n_glyphs):
        segs = []
        for k in range(n_rings):
            c = rng.uniform(size * 0.25, size * 0.75, 2)
            r0 = rng.uniform(size * 0.08, size * 0.35)
            a = np.sort(rng.uniform(0, 2 * np.pi, n_pts))
            r = r0 * (1 + jitter * rng.uniform(-1, 1, n_pts))
            pts = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)
            if k % 2:
                pts = pts[::-1]
            segs.append(ring(pts))
        segs = np.concatenate(segs)
        lo = np.floor(segs[:, [0, 1]].min(0)).astype(int) - 3
        hi = np.ceil(segs[:, [0, 1]].max(0)).astype(int) + 3
        out.append((segs, int(lo[0]), int(lo[1]), int(hi[0] - lo[0]), int(hi[1] - lo[1])))
    return out


# The input sets below are functions (glyphs_*) so that tests/raster_margin_sets.py can run the same inputs through the
# instances of the margins build (old_sets); every test renders exactly what its function returns.
def glyphs_random_small():
    rng = np.random.default_rng(1)
    return random_polys(rng, 40, 3, 40, 30)


def test_random_polygons_small(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_random_small())


def glyphs_random_multichunk():
    # N = 2600 and 5200 segments: 3 and 6 LDS chunks of the filtered kernel
    rng = np.random.default_rng(2)
    return random_polys(rng, 3, 2, 1300, 50) + random_polys(rng, 2, 4, 1300, 60)


def test_random_polygons_multichunk(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_random_multichunk())


def glyphs_overlapping_rings():
    sq = lambda a, b: [(a, a), (b, a), (b, b), (a, b)]  # noqa: E731
    ccw = ring(sq(2, 12))
    ccw2 = ring(sq(6, 16))
    cw = ring(sq(6, 16)[::-1])
    return [
        (np.concatenate([ccw, ccw2]), -1, -1, 20, 20),   # winding 2 in the overlap
        (np.concatenate([ccw, cw]), -1, -1, 20, 20),     # winding 0 in the overlap (XOR-like)
        (np.concatenate([ccw, ccw, ccw]), -1, -1, 16, 16),  # identical rings: ties everywhere
    ]


def test_overlapping_rings_winding(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_overlapping_rings())


def glyphs_on_vertices_and_rows():
    # vertices exactly on pixel centres (x.5), horizontal edges exactly on sample rows,
    # zero-length segments, a vertex repeated
    pts = [(2.5, 2.5), (9.5, 2.5), (9.5, 2.5), (9.5, 7.5), (6.5, 7.5), (6.5, 4.5), (2.5, 4.5)]
    segs = ring(pts)
    segs = np.concatenate([segs, [[4.5, 3.5, 4.5, 3.5]]])  # isolated degenerate segment
    return [(segs, 0, 0, 13, 11), (segs, -3, -2, 19, 15)]


def test_samples_on_vertices_and_rows(oracle, vg, ctx):
    glyphs = glyphs_on_vertices_and_rows()
    run_both(oracle, vg, ctx, glyphs)
    run_both(oracle, vg, ctx, glyphs[:1], mode=oracle.PRECISE)


def glyphs_many_ties():
    # 3000 copies of one small triangle: every segment copy ties -> >2048 survivors per tile
    tri = ring([(3, 3), (9, 4), (5, 9)])
    segs = np.tile(tri, (3000, 1))
    return [(segs, 0, 0, 12, 12)]


def test_many_ties_queue_overflow(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_many_ties())


def glyphs_on_rounding_boundaries():
    """axis-aligned edges at multiples of 1/64 px: 32 d is a multiple of 1/2 for most pixels, i.e.
    exactly ON the byte rounding boundary for half of them (the bounded-group kernel may only skip
    the f64 evaluation when the whole error interval is strictly inside one bin)"""
    glyphs = []
    for k in range(0, 64, 3):
        o = k / 64.0
        box = ring([(2 + o, 2 + o), (17 + o, 2 + o), (17 + o, 12 + o), (2 + o, 12 + o)])
        hole = ring([(5 + o, 5.5), (5 + o, 9.5), (14.5, 9.5 + o), (14.5, 5.5)])
        glyphs.append((np.concatenate([box, hole]), -1, -1, 22, 17))
    return glyphs


def test_distances_on_rounding_boundaries(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_on_rounding_boundaries())


def glyphs_finely_flattened():
    """what real fonts look like after flattening at 0.1 font units: hundreds of sub-pixel segments
    per ring, several 256-segment chunks, groups straddling ring boundaries and sharp corners"""
    rng = np.random.default_rng(11)
    glyphs = []
    for n_sub in (7, 37, 150):
        for _ in range(6):
            segs = []
            for k in range(3):
                c = rng.uniform(8, 16, 2)
                a = np.sort(rng.uniform(0, 2 * np.pi, 5))
                r = rng.uniform(2, 7, 5)
                corners = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)
                pts = []
                for i in range(5):
                    p, q = corners[i], corners[(i + 1) % 5]
                    t = np.linspace(0, 1, n_sub, endpoint=False)[:, None]
                    bulge = 0.6 * np.sin(np.pi * t) * np.array([[q[1] - p[1], p[0] - q[0]]]) / 8
                    pts.append(p + t * (q - p) + bulge)
                pts = np.concatenate(pts)
                segs.append(ring(pts if k % 2 == 0 else pts[::-1]))
            segs = np.concatenate(segs)
            lo = np.floor(segs[:, [0, 1]].min(0)).astype(int) - 3
            hi = np.ceil(segs[:, [0, 1]].max(0)).astype(int) + 3
            glyphs.append((segs, int(lo[0]), int(lo[1]), int(hi[0] - lo[0]), int(hi[1] - lo[1])))
    return glyphs


def test_finely_flattened_outlines(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_finely_flattened())


def glyphs_tall_localised_chunks():
    """tall bitmaps made of small finely flattened rings stacked vertically (and horizontally): each
    chunk of 256 segments is compact, so the default kernel skips most chunks per span by their boxes;
    rings straddling chunk and row-band boundaries, winding through skipped chunks' neighbours"""
    rng = np.random.default_rng(5)
    glyphs = []
    for n_rings, n_pts, vertical in ((7, 300, True), (5, 513, True), (6, 256, False), (9, 130, True)):
        segs = []
        for k in range(n_rings):
            c = (8.0 + rng.uniform(-1, 1), 10.0 + 17.0 * k) if vertical else (10.0 + 17.0 * k, 8.0 + rng.uniform(-1, 1))
            a = np.linspace(0, 2 * np.pi, n_pts, endpoint=False)
            r = 5.0 * (1 + 0.25 * np.sin(3 * a + k))
            pts = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)
            segs.append(ring(pts if k % 2 == 0 else pts[::-1]))
            if k == 2:  # a nested ring inside ring 2 (winding 0 / 2 depending on orientation)
                segs.append(ring(np.stack([c[0] + 2 * np.cos(a[::4]), c[1] + 2 * np.sin(a[::4])], 1)))
        segs = np.concatenate(segs)
        lo = np.floor(segs[:, [0, 1]].min(0)).astype(int) - 3
        hi = np.ceil(segs[:, [0, 1]].max(0)).astype(int) + 3
        glyphs.append((segs, int(lo[0]), int(lo[1]), int(hi[0] - lo[0]), int(hi[1] - lo[1])))
    return glyphs


def test_tall_glyphs_with_localised_chunks(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_tall_localised_chunks())


def glyphs_wide_and_thin():
    wide = ring(np.stack([np.linspace(5, 1500, 60), 6 + 3 * np.sin(np.linspace(0, 20, 60))], 1).tolist()
                + [(1500, 14), (5, 14)])
    thin = ring(np.stack([3 + 0.8 * np.sin(np.linspace(0, 9, 50)), np.linspace(4, 400, 50)], 1).tolist()
                + [(5.5, 400), (5.5, 4)])
    return [
        (wide, 0, 0, 1510, 20),    # w > 1023: histogram does not fit -> brute-force route
        (wide, 0, 0, 900, 20),     # clipped rect, filtered route, 2 rows per tile
        (thin, 0, 0, 7, 410),      # 7 px wide: 38 rows per tile
        (thin, -40, -40, 60, 30),  # rect mostly away from the outline
    ]


def test_wide_and_thin_rects(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_wide_and_thin())


def glyphs_big_and_far():
    rng = np.random.default_rng(4)
    base = random_polys(rng, 2, 2, 60, 24)
    glyphs = []
    for segs, x0, y0, w, h in base:
        for off in (1.0e4, 3.0e6 + 0.25, -7.0e8):
            s = segs.copy()
            s[:, [0, 2]] += off
            glyphs.append((s, x0 + int(np.floor(off)), y0, w, h))
        # segments far outside the rect (relative coordinates ~1e7: no usable f32 bound)
        glyphs.append((np.concatenate([segs, segs + 1.0e7]), x0, y0, w, h))
    return glyphs


def test_big_and_far_coordinates(oracle, vg, ctx):
    run_both(oracle, vg, ctx, glyphs_big_and_far())


def test_synthetic_first_outlines(oracle, vg, ctx):
    from versatiles_glyphs_rs_amd import synthetic as S
    batch = S.make_batch(0, 48)
    want, _ = oracle.sdf_render_batch(batch, oracle.PRECISE, 4)
    for variant in (0, 1):
        ctx.set_variant(variant)
        assert np.array_equal(ctx.render_batch(batch), want)
    ctx.set_variant(0)


def glyphs_tiny():
    tri = ring([(1, 1), (3, 1), (2, 3)])
    return [(tri, 0, 0, 1, 1), (tri, 0, 0, 4, 4), (tri[:0], 0, 0, 3, 3)]


def test_empty_and_tiny_batches(oracle, vg, ctx):
    assert ctx.render_batch(vg.make_batch([])).size == 0
    run_both(oracle, vg, ctx, glyphs_tiny())


def test_argument_validation(vg, ctx):
    b = vg.make_batch([(ring([(1, 1), (3, 1), (2, 3)]), 0, 0, 4, 4)])
    b.out_off[1] = 15  # inconsistent with w*h
    with pytest.raises(vg.VgsdfError) as e:
        ctx.render_batch(b)
    assert e.value.code == -1


def test_two_contexts_on_two_threads(oracle, vg):
    """vgsdf.h: one context per (host thread, GPU) — two threads with their own contexts (own streams,
    own device scratch) render different batches at the same time; each gets its own bytes"""
    import threading
    rng = np.random.default_rng(21)
    batches = [vg.make_batch(random_polys(rng, 60, 3, 50 + 30 * k, 28)) for k in range(2)]
    want = [oracle.sdf_render_batch(b, oracle.BRUTE, 4)[0] for b in batches]
    got, errs = [None, None], []

    def work(k):
        try:
            c = vg.SdfContext(0)
            for _ in range(20):
                got[k] = c.render_batch(batches[k])
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_only_product_variants_are_selectable(vg, ctx):
    """vgsdf_set_variant: 0 and 1 only; ablation / development ids fail with VGSDF_E_ARG."""
    for v in (2, 12, 13, 22, 23, 30, 31, 35, 45, 50, 51, 55, 57, -1, 1000):
        with pytest.raises(Exception):
            ctx.set_variant(v)
    ctx.set_variant(1)
    ctx.set_variant(0)
