"""Input sets for the SHAPES the span kernel's sweep takes (csrc/sdf_span_kernel.inc), not a test module.

Imported by tests/test_gpu_sweep_shapes.py and by its child process tests/sweep_shapes_child.py (the counting instance of the
margins build).  Every set is deterministic; a glyph is (segs[n, 4], x0, y0, w, h).

Phase 1 of a sweep treats a chunk's 32 groups in blocks of four: a full chunk (256 records) runs both passes in a straight line,
a partial chunk leaves the first pass at the first block past its groups and enters the second pass's switch at its block count.
Phase 2 deals the wave's (pixel, group) pairs out in rounds of 64 and reads a round's entry one round ahead; a wave whose pairs
pass the pool (QCAP = 256) lets every lane walk its own list instead."""
import numpy as np

CHUNK = 256   # records per chunk (FCHUNK)
GRP = 8       # records per group
QCAP = 256    # pooled pairs per wave and sweep

# one chunk: every block count 1 .. 8 of (n_groups + 3) / 4, empty groups inside the last real block, the full chunk
ONE_CHUNK = (1, 8, 9, 31, 32, 33, 57, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 248, 249, 255, 256)
# a full chunk (straight line) followed by a guarded one inside one workgroup, 257: a partial chunk of ONE group behind a full one
TWO_SHAPES = (257, 264, 288, 512, 513, 768 + 40)
# 16 x 16: one exactly full tile; 17 x 15: 255 px; 24 x 24: three tiles, the last a quarter full (three waves skip it)
WINDOWS = ((16, 16), (17, 15), (24, 24))


def blocks(n_seg):
    """blocks of four groups the last chunk of n_seg records holds"""
    last = n_seg - (n_seg - 1) // CHUNK * CHUNK
    return (-(-last // GRP) + 3) // 4


assert {blocks(n) for n in ONE_CHUNK} == set(range(1, 9)) and blocks(257) == 1 and blocks(768 + 40) == 2


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def jittered(n_seg, w, h, seed):
    """one closed ring of n_seg segments (n_seg = 1: a zero-length segment) around the middle of a w x h window, radius a third
    of the window, every vertex jittered in radius and angle"""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, n_seg, endpoint=False) + rng.uniform(-0.3, 0.3, n_seg) * (2 * np.pi / n_seg)
    r = min(w, h) / 3.0 * (1.0 + rng.uniform(-0.06, 0.06, n_seg))
    pts = np.stack([w / 2.0 + 0.13 + r * np.cos(a), h / 2.0 - 0.21 + r * np.sin(a)], 1)
    return (ring(pts), 0, 0, w, h)


def block_count_glyphs(counts):
    """one glyph per segment count, the windows in turn; then the first and the last count in the two windows they missed"""
    glyphs = [jittered(n, *WINDOWS[i % 3], seed=n) for i, n in enumerate(counts)]
    for n in (counts[0], counts[-1]):
        i = counts.index(n)
        glyphs += [jittered(n, *WINDOWS[(i + k) % 3], seed=n + 1000 * k) for k in (1, 2)]
    return glyphs


def smooth_64gon():
    """smooth 64-gons of radius 3 and 4 px in 24 x 24: 8 groups of 2 - 3 px; a pixel holds one or two candidate groups, a wave one
    or two rounds (the model of phase 1 on the CPU: 1.56 and 1.89 rounds per wave tile-chunk)"""
    a = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    return [(ring(np.stack([12.2 + r * np.cos(a), 11.8 + r * np.sin(a)], 1)), 0, 0, 24, 24) for r in (3.0, 4.0)]


def finely_flattened():
    """small shapes flattened far below a pixel, two laps of 128 segments 0.06 px apart (a stroke's two sides, a group a third
    of a pixel long): a pixel sees the groups of both laps at nearly the same distance; the waves across the shape take three to
    five rounds (the model of phase 1 on the CPU: 2.7 - 3.3 rounds per wave tile-chunk, a wave or two past the pool)"""
    glyphs = []
    for r, c in ((2.5, (11.7, 12.45)), (3.2, (12.3, 12.1)), (4.0, (12.05, 11.6))):
        laps = []
        for lap in range(2):
            a = np.linspace(0, 2 * np.pi, CHUNK // 2, endpoint=False) + 0.01 * lap
            rr = r + 0.06 * lap
            laps.append(ring(np.stack([c[0] + rr * np.cos(a) + 0.2 * np.sin(3 * a), c[1] + 0.8 * rr * np.sin(a)], 1)))
        glyphs.append((np.concatenate(laps), 0, 0, 24, 24))
    return glyphs


def many_ties():
    """100 copies of one small triangle (300 segments, two chunks): every group of the first chunk ties for every pixel, 32
    candidates per pixel, far past the pool"""
    tri = ring([(3, 3), (9, 4), (5, 9)])
    return [(np.tile(tri, (100, 1)), 0, 0, 12, 12)]


ROUND_SETS = {"smooth_64gon": smooth_64gon, "finely_flattened": finely_flattened, "many_ties": many_ties}
