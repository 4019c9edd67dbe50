"""CPU model of the stage's f32 decisions of sdf_tiles_span (development aid, numpy only, no GPU).

The stage needs two integers: per segment the bracket of sample rows it crosses, per (segment, row) pair the column of the
crossing.  The kernel takes the BRACKET from the f32 record where both end points lie farther than E_row (DESIGN.md §4.1,
"The stage's integers") from every integer, and from first_ge in f64 otherwise.  The same filter for the COLUMN (bound E_xc)
was built, measured slower and dropped; its restatement stays here (the xc_* figures) with the inputs that caught it.  This
file restates both in f32 (numpy float32, operation by operation) next to the f64 path and counts, over every segment and
every (segment, row) pair of a batch,

  * decisions of the f32 path that DIFFER from the f64 result (must be 0 with the margins in place),
  * the UNDECIDED share: lanes, pairs, and waves of 64 records / rounds of 64 pairs with at least one (these run the f64 path),
  * the same decisions with the margin set to 0 (VG_M_ROW_E := 0: the weakened instance of `make margins`), and for the columns
    that differ there, the distance of the flipped pixel from the segment (>= 1/64 px: a byte can change).

v_rcp_f32 is within 1 ulp of the quotient, not correctly rounded: every column figure is taken three times, with the rounded
reciprocal and with its two neighbours, and the worst is reported.

    python tools/model_stage_filters.py fira | noto_regular | noto_all | synthetic [max_glyphs]
    python tools/model_stage_filters.py sets          the directed sets of tests/stage_filter_sets.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

F = np.float32
U = F(2.0 ** -24)
ROW_C, ROW_ABS = F(6.0) * U, F(2.0 ** -22)
XC_C0, XC_C1, XC_ABS = F(16.0) * U, F(2.0) * U, F(2.0 ** -21)
M_MAX = F(1.0e6)
CHUNK, WAVE = 256, 64


def first_ge(v, c, A, B):
    """smallest integer n in [A, B] with n + c >= v (B if none), as sdf_span_support.h: exact f64 compares"""
    with np.errstate(invalid="ignore"):
        a = np.clip(np.ceil(v - c), A, B)
        n = np.where(np.isnan(a), A, a).astype(np.int64)
        down = (n > A) & ((n - 1).astype(np.float64) + c >= v)
        up = ~down & (n < B) & (n.astype(np.float64) + c < v)
    return n - down + up


def int_dist(t):
    fr = (t - np.floor(t)).astype(F)
    return np.minimum(fr, (F(1.0) - fr).astype(F))


def wave_max(a):
    """per record: the maximum over its wave of 64 records (a glyph's chunks of 256 start at multiples of 256)"""
    n = len(a)
    pad = np.concatenate([a, np.zeros((-n) % WAVE, a.dtype)]).reshape(-1, WAVE)
    return np.repeat(pad.max(axis=1), WAVE)[:n]


def glyph_model(segs, x0, y0, w, h):
    """counts of one glyph, rows 0 .. h - 1 as one span (a span's clamps only narrow these)"""
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    vx, vy, wx, wy = segs.T
    hw, hh = w >> 1, h >> 1
    ox, oy = float(x0 + hw), float(y0 + hh)
    x0c, y0c = x0 + 0.5, y0 + 0.5
    res = {}
    with np.errstate(all="ignore"):
        # ---- the f32 record, as the stage forms it ----
        fvx, fvy = (vx - ox).astype(F), (vy - oy).astype(F)
        fdx, fdy = (wx - vx).astype(F), (wy - vy).astype(F)
        mf = np.maximum(np.maximum(np.abs(fvx), np.abs(fvy)), np.maximum(np.abs(fvx + fdx), np.abs(fvy + fdy))) * F(1.00001)
        mf = np.where(mf >= 0, mf, F(np.inf)).astype(F)
        mpix = F(0.5) * F(max(w, h)) + F(1.0)
        # ---- rows: exact ----
        up = vy < wy
        lo, hi = np.where(up, vy, wy), np.where(up, wy, vy)
        ya = first_ge(lo, y0c, 0, h)
        yb = first_ge(hi, y0c, 0, h)
        nrow = np.where(vy != wy, np.maximum(yb - ya, 0), 0)
        # ---- rows: f32 ----
        tv, tw = (fvy - F(0.5)).astype(F), ((fvy + fdy).astype(F) - F(0.5)).astype(F)
        e_row = (ROW_C * np.maximum(mf, mpix) + ROW_ABS).astype(F)  # (one fma in the kernel: within the bound's slack)
        dist = np.minimum(int_dist(tv), int_dist(tw))
        cv, cw = np.ceil(tv), np.ceil(tw)
        ca = np.clip(np.minimum(cv, cw), 0 - hh, h - hh) + hh
        cb = np.clip(np.maximum(cv, cw), 0 - hh, h - hh) + hh
        f_nrow = cb - ca
        live = vy != wy
        for tag, e in (("", e_row), ("0", np.zeros_like(e_row))):
            dec = (dist > e) & (mf < M_MAX)
            und = live & ~dec
            bad = live & dec & ((f_nrow != nrow) | ((nrow > 0) & (ca != ya)))
            res["row_bad" + tag] = int(bad.sum())
            res["row_und" + tag] = int(und.sum())
            res["row_und_waves" + tag] = int((wave_max(und.astype(np.int64)) > 0)[::WAVE].sum())
        res["segs"] = len(vx)
        res["waves"] = -(-len(vx) // WAVE) if len(vx) else 0
        # ---- (segment, row) pairs from the exact brackets ----
        si = np.repeat(np.arange(len(vx)), nrow)
        if si.size == 0:
            res.update(pairs=0, rounds=0, xc_bad=0, xc_und=0, xc_und_rounds=0, xc_bad0=0, xc_und0=0, xc_vis0=0)
            return res
        first = np.cumsum(nrow) - nrow
        yy = ya[si] + (np.arange(si.size) - first[si])
        # exact: renderer_precise.rs:45-49, :63
        pyy = yy.astype(np.float64) + y0c
        dx, dy = wx - vx, wy - vy
        xc = vx[si] + ((pyy - vy[si]) / dy[si]) * dx[si]
        k = first_ge(xc, x0c, 0, w)
        # f32
        m_w = np.maximum(wave_max(mf), mpix)[si]
        c0 = np.where(m_w < M_MAX, (XC_C0 * m_w + XC_ABS).astype(F), F(np.inf)).astype(F)
        c1 = (XC_C1 * m_w).astype(F)
        ry = ((yy - hh).astype(F) + F(0.5)).astype(F)
        rcp0 = (F(1.0) / fdy[si]).astype(F)
        worst = dict(xc_bad=0, xc_und=0, xc_und_rounds=0, xc_bad0=0, xc_und0=0, xc_vis0=0)
        # rounds of 64 pairs: per wave of records, its pairs in order
        wave_of = si // WAVE
        rank = np.arange(si.size) - np.searchsorted(wave_of, wave_of, side="left")
        round_id = wave_of * 100000 + rank // WAVE
        res["pairs"] = int(si.size)
        res["rounds"] = int(np.unique(round_id).size)
        for rdy in (rcp0, np.nextafter(rcp0, F(np.inf)), np.nextafter(rcp0, F(-np.inf))):
            tc = ((ry - fvy[si]).astype(F) * rdy).astype(F)
            t = ((tc.astype(np.float64) * fdx[si].astype(np.float64) + fvx[si].astype(np.float64)).astype(F) - F(0.5)).astype(F)  # fma: one rounding
            e_xc = ((np.abs(fdx[si]) * np.abs(rdy)).astype(F) * c1 + c0).astype(F)
            d = int_dist(t)
            kf = np.clip(np.ceil(t), -hw, w - hw) + hw
            cur = {}
            for tag, e in (("", e_xc), ("0", np.zeros_like(e_xc))):
                dec = d > e
                bad = dec & (kf != k)
                cur["xc_bad" + tag] = int(bad.sum())
                cur["xc_und" + tag] = int((~dec).sum())
                if tag == "":
                    cur["xc_und_rounds"] = int(np.unique(round_id[~dec]).size)
                else:
                    # the pixel whose winding the wrong column flips: column min(kf, k) of row yy; its distance from the segment's line
                    col = np.minimum(kf, k)[bad]
                    px = col + x0c
                    ln = np.hypot(dx[si][bad], dy[si][bad])
                    perp = np.abs((px - vx[si][bad]) * dy[si][bad] - (pyy[bad] - vy[si][bad]) * dx[si][bad]) / ln
                    cur["xc_vis0"] = int((perp >= 1.0 / 64.0 + 1.0e-3).sum())
            for key in ("xc_bad", "xc_und", "xc_und_rounds", "xc_und0"):
                worst[key] = max(worst[key], cur[key])
            worst["xc_bad0"] = cur["xc_bad0"] if rdy is rcp0 else min(worst["xc_bad0"], cur["xc_bad0"])  # the weakened kernel must fail whatever v_rcp_f32 returns
            worst["xc_vis0"] = cur["xc_vis0"] if rdy is rcp0 else min(worst["xc_vis0"], cur["xc_vis0"])
        res.update(worst)
    return res


def batch_model(glyphs):
    tot = {}
    for g in glyphs:
        if len(g[0]) and g[3] * g[4] > 0:
            for key, v in glyph_model(*g).items():
                tot[key] = tot.get(key, 0) + v
    return tot


def font_glyphs(workload, max_glyphs=None):
    from conftest import FIRA, NOTO, load_product, noto_files
    vg = load_product()
    if workload == "synthetic":
        from versatiles_glyphs_rs_amd import synthetic as S
        b = S.make_batch(0, max_glyphs or 256)
    else:
        name, files = {"fira": ("Fira Sans Regular", [FIRA]), "noto_regular": ("Noto Sans Regular", [NOTO]),
                       "noto_all": ("Noto Sans Regular", None)}[workload]
        mgr = vg.FontManager(True)
        fid = mgr.add_font_with_name(name, files or noto_files())
        hb = mgr.build_batch(fid)  # keep the owner alive: the arrays are views into its memory
        b = hb.batch
    n = b.n_glyphs if max_glyphs is None else min(b.n_glyphs, max_glyphs)
    out = []
    for g in range(n):
        a, e = int(b.seg_off[g]), int(b.seg_off[g + 1])
        segs = np.stack([b.seg_sx[a:e], b.seg_sy[a:e], b.seg_ex[a:e], b.seg_ey[a:e]], 1).copy()
        out.append((segs, int(b.x0[g]), int(b.y0[g]), int(b.w[g]), int(b.h[g])))
    return out


def report(name, m):
    def pct(a, b):
        return f"{100.0 * a / b:6.3f} %" if b else "   -    "
    print(f"{name}: {m.get('segs', 0)} segments in {m.get('waves', 0)} waves, {m.get('pairs', 0)} (segment, row) pairs in {m.get('rounds', 0)} rounds")
    print(f"  rows:    differing {m.get('row_bad', 0)}   undecided lanes {m.get('row_und', 0)} ({pct(m.get('row_und', 0), m.get('segs', 0))})"
          f"   waves with one {m.get('row_und_waves', 0)} ({pct(m.get('row_und_waves', 0), m.get('waves', 0))})")
    print(f"  columns: differing {m.get('xc_bad', 0)}   undecided pairs {m.get('xc_und', 0)} ({pct(m.get('xc_und', 0), m.get('pairs', 0))})"
          f"   rounds with one {m.get('xc_und_rounds', 0)} ({pct(m.get('xc_und_rounds', 0), m.get('rounds', 0))})")
    print(f"  margins := 0: rows differing {m.get('row_bad0', 0)}; columns differing {m.get('xc_bad0', 0)}, "
          f"of them {m.get('xc_vis0', 0)} with the flipped pixel >= 1/64 px from the segment")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "fira"
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else None
    if what == "sets":
        import stage_filter_sets as S
        for name, glyphs in S.sets().items():
            report(name, batch_model(glyphs))
    else:
        report(what, batch_model(font_glyphs(what, cap)))


if __name__ == "__main__":
    main()
