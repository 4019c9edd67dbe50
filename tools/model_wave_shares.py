"""CPU model of how the span kernel's sweep work falls on the four waves of a workgroup, by wave index.

Thread tid of a workgroup owns pixel p0 + k*256 + ((tid + 64*rot) & 255) of tile k; a wave whose 64 pixels all lie past the
end of the bitmap skips the sweep.  Only a glyph's last tile is partial and its empty quarters are the last ones, so with
rot = 0 everywhere (the kernel before the rotation) the high wave indices sweep less.  This model rebuilds the host planner's
work list (work_plan.h's policy, work_list.cpp's order and deal over the XCD queues: restated here on purpose), counts the
tile-chunk sweeps per wave index with rot = 0 and with the kernel's hash (sdf_span_support.h, wave_rot), and checks the hash:

  max over mean of the four per-wave-index totals                                   <= 1.02 on every batch
  the same inside every block of 32 consecutive work-list positions of one XCD
  residue (blockIdx % 8), averaged over the blocks (weighted by their sweeps)        <= 1.05

(A chunk the chunk-box test skips is counted as swept: the test is per workgroup, the same for its four waves.)

    python tools/model_wave_shares.py [fira noto_regular noto_all]      exit status 1 if a condition fails
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

WORK = {"fira": "Fira Sans Regular", "noto_regular": "Noto Sans Regular", "noto_all": "Noto Sans Regular"}
WAVE_ROT_MUL = 0x13C6EF37  # sdf_span_support.h
DELTA_CAP, SPAN_MAX = 2048, 4
LIMIT_ALL, LIMIT_BLOCK = 1.02, 1.05


def wave_rot(b, mul=WAVE_ROT_MUL):
    return ((b * mul) & 0xFFFFFFFF) >> 30


def span_fits(w, T):
    return ((256 * T - 2) // w + 2) * (w + 2) <= DELTA_CAP


def plan_glyph(px, w, n_seg, budget):
    """work_plan.h, plan_glyph: (class, T, weight)"""
    if not span_fits(w, 1) or n_seg >= 1 << 24:
        cls, T = 1, 1
    else:
        cls = 0
        chunks = (n_seg + 255) // 256
        T = min(SPAN_MAX, max(budget // max(chunks, 1), 1))
        while T > 1 and not span_fits(w, T):
            T -= 1
    t256 = (px + 255) >> 8
    return cls, T, min(n_seg * min(t256, T), 0xFFFFFFFF)


def weight_bucket(weight):
    if weight < 16:
        return 511 - weight
    e = weight.bit_length() - 1
    return 511 - ((e - 3) * 16 + ((weight >> (e - 4)) & 15))


def work_list(w, h, n_seg):
    """The main class of work_list.cpp's list: [(glyph, first pixel, tiles)] in dispatch order (position = blockIdx.x)."""
    n = len(w)
    budget = 8 if n < 2048 else 16
    keys, span_t = [], {}
    for g in range(n):
        px = int(w[g]) * int(h[g])
        if px == 0:
            continue
        cls, T, weight = plan_glyph(px, int(w[g]), int(n_seg[g]), budget)
        if cls == 0:
            span_t[g] = T
            keys.append((weight_bucket(weight), g))
    keys.sort(key=lambda k: k[0])  # stable: glyph order inside a bucket

    def emit(g):
        px, T = int(w[g]) * int(h[g]), span_t[g]
        return [(g, p, min(T, (px - p + 255) >> 8)) for p in range(0, px, 256 * T)]

    total = sum(len(emit(g)) for _, g in keys)
    if total < 64:
        return [e for _, g in keys for e in emit(g)]
    queues = [[] for _ in range(8)]
    for _, g in keys:
        min(queues, key=len).extend(emit(g))  # the first of the shortest queues
    taken, out = [0] * 8, []
    while len(out) < total:
        for k in range(8):
            if len(out) == total:
                break
            src = k
            if taken[src] >= len(queues[src]):
                for m in range(8):  # dry: borrow from the fullest queue
                    if len(queues[m]) - taken[m] > len(queues[src]) - taken[src]:
                        src = m
            out.append(queues[src][taken[src]])
            taken[src] += 1
    return out


def sweeps_by_slot(entries, w, h, n_seg):
    """per work-list position: tile-chunk sweeps of the four 64-pixel quarters of its tiles, and its chain (chunks x tiles)"""
    q = np.zeros((len(entries), 4), dtype=np.int64)
    chain = np.zeros(len(entries), dtype=np.int64)
    for i, (g, p, T) in enumerate(entries):
        npix, chunks = int(w[g]) * int(h[g]), (int(n_seg[g]) + 255) // 256
        chain[i] = chunks * T
        for k in range(T):
            for s in range(4):
                if p + k * 256 + s * 64 < npix:
                    q[i, s] += chunks
    return q, chain


def by_wave(q, rot):
    """wave wv takes quarter (wv + rot) & 3"""
    idx = (np.arange(4)[None, :] + rot[:, None]) & 3
    return np.take_along_axis(q, idx, axis=1)


def spread(tot):
    return float(tot.max() / tot.mean()) if tot.sum() else 1.0


def block_spread(per_wave):
    """max over mean inside blocks of 32 consecutive positions of one XCD residue, averaged with the blocks' sweeps as weights"""
    num = den = 0.0
    for r in range(8):
        rows = per_wave[r::8]
        for a in range(0, len(rows), 32):
            t = rows[a:a + 32].sum(axis=0)
            if t.sum():
                num += spread(t) * t.sum()
                den += t.sum()
    return num / den if den else 1.0


def model(w, h, n_seg, mul=WAVE_ROT_MUL):
    entries = work_list(w, h, n_seg)
    q, chain = sweeps_by_slot(entries, w, h, n_seg)
    b = np.arange(len(entries), dtype=np.uint64)
    rot = ((b * np.uint64(mul)) & np.uint64(0xFFFFFFFF)) >> np.uint64(30)
    today, rotated = by_wave(q, np.zeros(len(entries), dtype=np.int64)), by_wave(q, rot.astype(np.int64))
    return {"workgroups": len(entries), "chain": chain, "today": today, "rotated": rotated}


def batch_shapes(workload):
    from conftest import FIRA, NOTO, load_product, noto_files
    files = {"fira": [FIRA], "noto_regular": [NOTO], "noto_all": None}[workload] or noto_files()
    vg = load_product()
    mgr = vg.FontManager(True)
    hb = mgr.build_batch(mgr.add_font_with_name(WORK[workload], files))
    b = hb.batch  # (copies: the batch's arrays live as long as hb)
    return np.array(b.w, dtype=np.int64), np.array(b.h, dtype=np.int64), np.diff(np.array(b.seg_off, dtype=np.int64))


def main():
    ok = True
    for workload in sys.argv[1:] or ["noto_regular", "fira", "noto_all"]:
        w, h, n_seg = batch_shapes(workload)
        m = model(w, h, n_seg)
        vals, cnt = np.unique(m["chain"], return_counts=True)
        top = ", ".join(f"{v}:{c}" for v, c in list(zip(vals, cnt))[::-1][:5])
        print(f"{workload}: {len(w)} glyphs, {m['workgroups']} workgroups; longest chains (tile-chunks:workgroups) {top}")
        for name in ("today", "rotated"):
            tot = m[name].sum(axis=0)
            print(f"  {name:8s} sweeps by wave index {' '.join(f'{int(t):7d}' for t in tot)}   share of wave 0 "
                  f"{' '.join(f'{t / max(tot[0], 1):.2f}' for t in tot)}   max/mean {spread(tot):.3f}   in blocks of 32 per XCD {block_spread(m[name]):.3f}")
        tot = m["rotated"].sum(axis=0)
        good = spread(tot) <= LIMIT_ALL and block_spread(m["rotated"]) <= LIMIT_BLOCK
        print(f"  hash (b * 0x{WAVE_ROT_MUL:08X}) >> 30: max/mean <= {LIMIT_ALL} and <= {LIMIT_BLOCK} in blocks: {'ok' if good else 'FAILED'}")
        ok = ok and good
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
