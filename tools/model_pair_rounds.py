"""CPU model of phase 2's pair rounds of sdf_tiles_span (development aid, numpy only, no GPU).

Restates phase 1's candidate rule as tools/model_candidates.py does (`seq`: the bound from the chunk's own anchors and the one
carried from earlier chunks) on a font's tessellated batch (product host stage) and keeps, per wave tile-chunk SWEEP, the
number of (pixel, group) pairs and the busiest lane's.  From those it prints what the pair rounds are made of:

  * sweeps, pairs, the sweeps above the pool's capacity QCAP with their pairs and their busiest lane;
  * the histogram of the last round's entries of the pooled sweeps (0, 1-16, 17-32, 33-64);
  * the sweeps without any pair;
  * VALU instructions per sweep under four policies, from the per-round costs below.

    python tools/model_pair_rounds.py noto_regular [max_glyphs]

The chunk-box skip is not modelled (the counting build sweeps 0.3 % fewer wave tile-chunks on Noto Sans Regular).
profiles/pair_rounds_ab.txt holds the figures next to the counting build's and what the GPU made of the policies."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import FIRA, NOTO, load_product, noto_files  # noqa: E402

WORK = {"fira": ("Fira Sans Regular", [FIRA]), "noto_regular": ("Noto Sans Regular", [NOTO]),
        "noto_all": ("Noto Sans Regular", None)}
INFL = 1 + 1 / 512
GRP = 8
CH = 256
QCAP = 256
# VALU instructions, read from the kernel's assembly (make asm)
ROUND = 87          # a full round: 8 filters, the bpermutes' addresses, the merge
HALF_ROUND = 54     # a half round: 4 filters per lane, the swap, the guard
QUARTER_ROUND = 40  # a quarter round as costed (not built): 2 filters per lane
WALK_GROUP = 83     # one group of a lane's own walk
NO_PAIR = 35        # what a sweep without a pair runs behind phase 1: scan, pool set-up, decide, ballot, byte update (30 - 40)


def seg_dist2(px, py, sx, sy, ex, ey):
    """squared distances pixels x segments"""
    dx, dy = ex - sx, ey - sy
    l2 = dx * dx + dy * dy
    pvx = px[:, None] - sx[None, :]
    pvy = py[:, None] - sy[None, :]
    t = np.clip((pvx * dx + pvy * dy) / np.where(l2 > 0, l2, 1), 0, 1)
    qx = pvx - t * dx
    qy = pvy - t * dy
    return qx * qx + qy * qy


def glyph_sweeps(sx, sy, ex, ey, w, h):
    """(total, busiest lane's pairs) of every wave tile-chunk sweep of one glyph (coordinates relative to the bitmap's corner)"""
    npix = w * h
    o = np.arange(npix)
    row = o // w
    px = (o - row * w) + 0.5
    py = (h - 1 - row) + 0.5
    d2 = seg_dist2(px, py, sx, sy, ex, ey)
    nseg = len(sx)
    M = max(np.abs(np.concatenate([sx, sy, ex, ey])).max(), w, h)
    pad = 0.01 + 1e-5 * M
    padn = -(-npix // 256) * 256
    act = np.arange(padn).reshape(-1, 64)[:, 0] < npix
    ub2 = np.full(npix, np.inf)
    out = []
    for c0 in range(0, nseg, CH):
        c1 = min(nseg, c0 + CH)
        cnt = c1 - c0
        ng = -(-cnt // GRP)
        ax, ay, r = np.empty(ng), np.empty(ng), np.empty(ng)
        for k in range(ng):
            gb = k * GRP
            ai = min(gb + GRP // 2, cnt - 1)
            ax[k], ay[k] = sx[c0 + ai], sy[c0 + ai]
            m0, m1 = c0 + gb, min(c0 + gb + GRP, c1)
            rr = np.maximum((sx[m0:m1] - ax[k]) ** 2 + (sy[m0:m1] - ay[k]) ** 2, (ex[m0:m1] - ax[k]) ** 2 + (ey[m0:m1] - ay[k]) ** 2).max()
            r[k] = (np.sqrt(rr) * INFL + pad) * INFL * 1.004
        D2 = (px[:, None] - ax[None, :]) ** 2 + (py[:, None] - ay[None, :]) ** 2
        dmin = np.minimum(ub2, D2.min(axis=1))
        U = np.minimum((np.sqrt(dmin) * INFL + pad) * INFL, 6.2) * 1.004
        cand = (U[:, None] + r[None, :]) ** 2 - D2 * (1 - 2.0 ** -8) >= 0  # bf16 truncation of D2: up to 2^-7 smaller
        cw = np.zeros(padn, dtype=np.int64)
        cw[:npix] = cand.sum(axis=1)
        cw = cw.reshape(-1, 64)[act]
        out.append(np.stack([cw.sum(axis=1), cw.max(axis=1)], 1))
        segmask = np.repeat(cand, GRP, axis=1)[:, :cnt]
        f1 = np.where(segmask, d2[:, c0:c1], np.inf).min(axis=1)
        ub2 = np.minimum(ub2, np.minimum(dmin, f1 * (1 + 1e-6)))   # the carried bound: the chunk's candidate minimum
    return np.concatenate(out)


def sweeps_of(workload, max_glyphs=None):
    vg = load_product()
    name, files = WORK[workload]
    mgr = vg.FontManager(True)
    fid = mgr.add_font_with_name(name, files or noto_files())
    hb = mgr.build_batch(fid)  # keep the owner alive: the arrays are views into its memory
    b = hb.batch
    n = b.n_glyphs if max_glyphs is None else min(b.n_glyphs, max_glyphs)
    out = [np.zeros((0, 2), dtype=np.int64)]
    for g in range(n):
        a, e = int(b.seg_off[g]), int(b.seg_off[g + 1])
        w, h, x0, y0 = int(b.w[g]), int(b.h[g]), int(b.x0[g]), int(b.y0[g])
        if e > a and w * h > 0:
            out.append(glyph_sweeps(b.seg_sx[a:e] - x0, b.seg_sy[a:e] - y0, b.seg_ex[a:e] - x0, b.seg_ey[a:e] - y0, w, h))
    return n, np.concatenate(out)


def window_costs(n, half, quarter):
    """VALU of the rounds over n <= QCAP pooled entries"""
    if n == 0:
        return 0
    tail = (n - 1) % 64 + 1
    last = QUARTER_ROUND if quarter and tail <= 16 else HALF_ROUND if half and tail <= 32 else ROUND
    return (n - tail) // 64 * ROUND + last


def model(sweeps):
    """the figures of a set of sweeps (rows: total, busiest lane's pairs)"""
    total, busiest = sweeps[:, 0], sweeps[:, 1]
    over = total > QCAP
    pooled = total[~over]
    tail = np.where(pooled == 0, 0, (pooled - 1) % 64 + 1)
    fig = {"sweeps": len(total), "pairs": int(total.sum()), "rounds": int((-(-total // 64)).sum()),
           "over": int(over.sum()), "over_pairs": int(total[over].sum()), "over_max": int(total.max(initial=0)),
           "over_busiest": float(busiest[over].mean()) if over.any() else 0.0,
           "over_mean_lane": float(total[over].mean() / 64) if over.any() else 0.0,
           "no_pair": int((total == 0).sum()),
           "tails": {"0": int((tail == 0).sum()), "1-16": int(((tail >= 1) & (tail <= 16)).sum()),
                     "17-32": int(((tail >= 17) & (tail <= 32)).sum()), "33-64": int((tail >= 33).sum())}}

    def cost(passes, half, quarter):
        c = 0
        for t, bz in zip(total.tolist(), busiest.tolist()):
            if t > QCAP and not passes:
                c += bz * WALK_GROUP
            else:
                c += sum(window_costs(min(QCAP, t - b), half, quarter) for b in range(0, t, QCAP))
        return c / max(len(total), 1)

    fig["valu_per_sweep"] = {"today": cost(False, False, False), "passes": cost(True, False, False),
                             "half": cost(True, True, False), "quarter": cost(True, True, True),
                             "half, walk kept": cost(False, True, False)}
    fig["no_pair_valu_per_sweep"] = NO_PAIR * fig["no_pair"] / max(len(total), 1)
    return fig


def main():
    workload = sys.argv[1]
    n, sweeps = sweeps_of(workload, int(sys.argv[2]) if len(sys.argv) > 2 else None)
    f = model(sweeps)
    s = max(f["sweeps"], 1)
    print(f"{workload}: {n} glyphs, {f['sweeps']} wave tile-chunk sweeps, {f['pairs']} pairs, {f['rounds']} rounds")
    print(f"  above QCAP = {QCAP}: {f['over']} sweeps ({100 * f['over'] / s:.1f} %), {f['over_pairs']} pairs "
          f"({100 * f['over_pairs'] / max(f['pairs'], 1):.1f} %), mean {f['over_pairs'] / max(f['over'], 1):.0f}, largest {f['over_max']}; "
          f"busiest lane {f['over_busiest']:.1f} groups against a mean of {f['over_mean_lane']:.1f}")
    pooled = max(f["sweeps"] - f["over"], 1)
    print("  last round of the pooled sweeps: " + ", ".join(f"{k} entries {v} ({100 * v / pooled:.1f} %)" for k, v in f["tails"].items()))
    print(f"  sweeps without a pair: {f['no_pair']} ({100 * f['no_pair'] / s:.1f} %), ~{f['no_pair_valu_per_sweep']:.1f} VALU per sweep "
          f"at {NO_PAIR} each")
    print(f"  VALU per sweep in the rounds (round {ROUND}, half {HALF_ROUND}, quarter {QUARTER_ROUND}, walk {WALK_GROUP} per group): "
          + ", ".join(f"{k} {v:.1f}" for k, v in f["valu_per_sweep"].items()))


if __name__ == "__main__":
    main()
