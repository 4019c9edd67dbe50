"""Input sets for phase 2's pair rounds of the span kernel (csrc/sdf_span_kernel.inc), not a test module.

Imported by tests/test_pair_round_sets_host.py (CPU: every set has the figures it claims), tests/test_gpu_pair_rounds.py and its
child process tests/pair_round_child.py (the counting instance of the margins build).  Deterministic; a glyph is
(segs[n, 4], x0, y0, w, h).  No font.

A wave pools its (pixel, group) pairs and deals them out in rounds of 64: a last round of at most 32 entries is a half round
(two lanes per entry, four records each), in a sweep of more than QCAP pairs every lane walks its own list, and a wave
without any pair leaves the sweep behind phase 1.  (The totals past QCAP are also the window edges of a sweep pooled in passes
of QCAP pairs: built, measured slower than the walk and not kept, profiles/pair_rounds_ab.txt.)  A sweep's total is set exactly by arithmetic:

  * a bitmap of L <= 64 pixels is one wave with L owning lanes (or the last tile of a taller bitmap: 256 k + L pixels);
  * an outline of G groups with ONE far vertex has a coordinate bound M in [4096, 10^6): the group bounds are switched off,
    every group is a candidate of every owning lane, and the wave's total is L G.

The other sets stay in the bounded regime (M < 4096), where a decided pixel's byte comes straight from the pooled minimum."""
import numpy as np

CHUNK = 256   # records per chunk (FCHUNK)
GRP = 8       # records per group
QCAP = 256    # pooled pairs per wave and sweep
FAR = (6000.25, -5000.5)   # the far vertex: 4096 <= M < 10^6

# total -> (L, G): the table of the totals to cover
TOTALS = {1: (1, 1), 16: (16, 1), 17: (17, 1), 31: (31, 1), 32: (32, 1), 33: (33, 1), 63: (63, 1), 64: (64, 1), 65: (13, 5),
          96: (32, 3), 99: (33, 3), 256: (64, 4), 258: (43, 6), 288: (36, 8), 289: (17, 17), 512: (64, 8), 513: (27, 19),
          660: (60, 11), 2048: (64, 32)}
assert all(L * G == t and L <= 64 and G <= CHUNK // GRP for t, (L, G) in TOTALS.items())


def ring(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def window(L):
    """w x h = L with h the largest divisor of L up to 8"""
    h = max(d for d in range(1, 9) if L % d == 0)
    return L // h, h


def wobbly(n_seg, cx, cy, r, seed):
    """a closed ring of n_seg segments around (cx, cy), every vertex jittered in radius and angle"""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, n_seg, endpoint=False) + rng.uniform(-0.3, 0.3, n_seg) * (2 * np.pi / n_seg)
    rr = r * (1.0 + rng.uniform(-0.06, 0.06, n_seg))
    return np.stack([cx + 0.13 + rr * np.cos(a), cy - 0.21 + rr * np.sin(a)], 1)


def far_glyph(w, h, G, last=GRP, seed=0):
    """G groups (the last one of `last` records) around the middle of a w x h window, the middle vertex moved far away"""
    n = GRP * (G - 1) + last
    pts = wobbly(n, w / 2.0, h / 2.0, max(min(w, h) / 3.0, 0.8), seed)
    pts[n // 2] = FAR
    return (ring(pts), 0, 0, w, h)


def far_total(total):
    L, G = TOTALS[total]
    return [far_glyph(*window(L), G, seed=total)]


# ---- numpy restatement of what fixes a sweep's total: the groups of a chunk, the coordinate bound, the owning lanes ----

def n_groups(n_seg):
    """groups per chunk of an outline of n_seg records"""
    return [-(-min(CHUNK, n_seg - c0) // GRP) for c0 in range(0, n_seg, CHUNK)]


def coord_bounds(glyph):
    """the kernel's coordinate bound Mc per chunk: f32 records relative to the middle of the bitmap (an integer point), the
    end point as v + d, rounded up by 1.00001; at least 0.5 max(w, h) + 1"""
    segs, x0, y0, w, h = glyph
    f = np.float32
    ox, oy = x0 + w // 2, y0 + h // 2
    vx, vy = (segs[:, 0] - ox).astype(f), (segs[:, 1] - oy).astype(f)
    dx, dy = (segs[:, 2] - segs[:, 0]).astype(f), (segs[:, 3] - segs[:, 1]).astype(f)
    m = np.maximum(np.maximum(np.abs(vx), np.abs(vy)), np.maximum(np.abs(vx + dx), np.abs(vy + dy))) * f(1.00001)
    mpix = f(0.5) * f(max(w, h)) + f(1.0)
    return [float(max(m[c0:c0 + CHUNK].max(), mpix)) for c0 in range(0, len(segs), CHUNK)]


def owning_lanes(w, h):
    """owning lanes of every wave that holds a pixel (a wave = 64 consecutive pixels of a 256-pixel tile)"""
    npix = w * h
    return [min(64, npix - p) for p in range(0, npix, 64)]


def far_counters(glyphs):
    """what the counting instance counts on glyphs whose every chunk is unbounded: every group a candidate of every owning lane"""
    totals = [L * g for segs, _, _, w, h in glyphs for g in n_groups(len(segs)) for L in owning_lanes(w, h)]
    return {"pairs": sum(totals), "rounds": sum(-(-t // 64) for t in totals), "wave_tile_chunks": len(totals),
            "pool_overflows": sum(t > QCAP for t in totals)}


def nearest_records(glyph):
    """per pixel: index of the record with the smallest exact squared distance (f64)"""
    segs, x0, y0, w, h = glyph
    o = np.arange(w * h)
    px, py = x0 + o % w + 0.5, y0 + (h - 1 - o // w) + 0.5
    sx, sy, ex, ey = segs.T
    dx, dy = ex - sx, ey - sy
    l2 = dx * dx + dy * dy
    t = np.clip(((px[:, None] - sx) * dx + (py[:, None] - sy) * dy) / np.where(l2 > 0, l2, 1), 0, 1)
    qx, qy = px[:, None] - sx - t * dx, py[:, None] - sy - t * dy
    return np.argmin(qx * qx + qy * qy, axis=1)


# ---- further sets ----

def straddle():
    """289 = 17 x 17: 256 is no multiple of 17, so lane 15's entries 255 .. 271 straddle QCAP; its nearest record lies in one of
    its later groups (behind the boundary)"""
    return far_total(289)


def winner_halves():
    """bounded regime, ONE group of eight records (an octagon) in a 6 x 5 window: 30 pairs, a half round; around the octagon the
    nearest record is each of the eight in turn, so the minimum comes from either half of the group"""
    a = np.linspace(0, 2 * np.pi, 8, endpoint=False) + 0.1
    return [(ring(np.stack([3.1 + 1.6 * np.cos(a), 2.4 + 1.5 * np.sin(a)], 1)), 0, 0, 6, 5)]


def short_last_group(regime):
    """the last group holds 1, 2 and 3 records (the rest of it is padding, F = 2e36, which must never win): 9, 10 and 11
    segments in a 4 x 4 window, 16 lanes x 2 groups = 32 pairs, a half round.  `far`: the total by arithmetic; `near`: bounded"""
    glyphs = []
    for t in (1, 2, 3):
        if regime == "far":
            glyphs.append(far_glyph(4, 4, 2, last=t, seed=40 + t))
        else:
            glyphs.append((ring(wobbly(GRP + t, 2.0, 2.0, 1.4, 50 + t)), 0, 0, 4, 4))
    return glyphs


def padding_lanes():
    """23 x 12 = 256 + 20 pixels, one group: the last tile's wave has 20 owning lanes and 44 padding lanes, a half round of 20"""
    return [far_glyph(23, 12, 1, seed=7)]


def padding_lanes_passes():
    """23 x 12 with 14 groups: full waves of 896 pairs, the last tile's wave 280 (20 owning lanes): all past the pool"""
    return [far_glyph(23, 12, 14, seed=8)]


def _two_chunks(near_first):
    near = ring(wobbly(CHUNK, 6.0, 6.0, 3.5, 11))
    away = ring(wobbly(GRP, 60.0, 70.0, 2.0, 12))   # > 50 px from every pixel: beyond SAT + any radius, and M stays < 4096
    if near_first:
        return [(np.concatenate([near, away]), 0, 0, 12, 12)]
    return [(np.concatenate([np.tile(away, (CHUNK // GRP, 1)), near]), 0, 0, 12, 12)]


def no_pair_behind():
    """bounded regime, two chunks: the second chunk is out of every pixel's reach, so its sweeps find no pair after a chunk with pairs"""
    return _two_chunks(True)


def no_pair_first():
    """the reverse order: no pair in the first chunk (the carried bound is still infinite), pairs in the second"""
    return _two_chunks(False)


FAR_SETS = {f"total_{t:04d}": (lambda t=t: far_total(t)) for t in TOTALS}
FAR_SETS.update({"short_last_group_far": lambda: short_last_group("far"), "padding_lanes": padding_lanes,
                 "padding_lanes_passes": padding_lanes_passes})
NEAR_SETS = {"winner_halves": winner_halves, "short_last_group_near": lambda: short_last_group("near"),
             "no_pair_behind": no_pair_behind, "no_pair_first": no_pair_first}
SETS = {**FAR_SETS, **NEAR_SETS}
