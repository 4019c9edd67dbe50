// outline_kernels.hip — the flattening pipeline of the device front-end: outline commands ->
// flattened, closed rings -> scaled + shifted segments and the raster rect of every glyph,
// all on the GPU, bit-exact with the host/reference path:
//   RingBuilder          /root/reference/src/render/ring_builder.rs:26-117
//   add_quadratic_bezier / add_cubic_bezier   src/geometry/ring.rs:119-187
//   Ring::close          src/geometry/ring.rs:53-63
//   rings.scale / translate / get_bbox       src/geometry/rings.rs:50-70, point.rs:83-99
//   Renderer::prepare_glyph                  src/render/renderer.rs:64-91
//   Rings::get_segments                      src/geometry/rings.rs:75-81
// The host only parses font tables and records the OutlineBuilder callbacks (f32 font
// units); everything after that is f64 arithmetic replayed here operation by operation
// (-ffp-contract=off, IEEE divide).
//
// Pipeline: five launches, no intermediate point arrays, one read-back (the rects) for the host; four of them are here:
//   context  wave per glyph: is the ring non-empty in front of every command; commands that arrive in the compact
//            upload form (kind byte + the coordinates the kind carries) are expanded into 28-byte records here
//   count    wave per 64 commands: first flattening pass — how many points every command appends, their
//            bounding box (nothing else is stored)
//   rings    wave per glyph: point offsets inside the glyph, ring acceptance / closing rules, segment count,
//            bbox -> rect
//   plan     one workgroup: segment / output offsets of all glyphs (descriptors), the raster's work list
//            (spans, heaviest first), totals — outline_plan_kernels.hip
//   emit     wave per 64 commands: second flattening pass; every point goes straight into the scaled + shifted
//            segment records as the start of one segment and the end of its predecessor
// The two flattening passes deal the points of 64 consecutive commands out to the 64 lanes of a wave in items
// of up to 8 points ("Leaf-parallel flattening" below); one command per thread left 63 lanes waiting for the
// lane with a 32-point curve (36 + 45 us per Noto Sans Regular font; now 7 + 21), and a wave-per-glyph form
// measured 2.5x slower still.
// How the commands come to be on the device in the first place (the glyf decoder, the uploads of resident and ranges
// submissions) is input_form_kernels.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "outline_kernels.h"
#include "sdf_kernels.h"
#include "wave_ops.h"

namespace vgsdf {

constexpr double kTolSq = 0.01; // ring_builder.rs:62 `precision`, passed as tolerance_sq (:91,:108)
constexpr int kMaxStack = 18;   // the work list holds at most this many pending halves; flatness shrinks 4x per level,
                                // so that covers control polygons up to ~4e8 font units
constexpr uint32_t kMaxCurvePoints = 1u << 17;
// Non-finite or absurd control points never become flat (the reference would not terminate, or would emit
// ~2^52 points): a curve stops subdividing once its work list is full or it has emitted kMaxCurvePoints points;
// what is still pending then emits its end point only, so a curve yields at most kMaxCurvePoints + kMaxStack
// points and every loop below ends.  (A full work list alone does not bound the loop: the right spine of the
// subdivision tree is reached with an empty list at any depth.)

// Iterative de Casteljau, explicit LIFO stack, right half pushed first (ring.rs:119-144).
// Calls emit(x, y) for every point appended to the ring, in order.  Returns the count.
//
// The reference pushes (m, m2, e) then (s, m1, m) and pops the left half at once; what stays on its
// stack are the right halves of the ancestors.  A right half's start point is the end point of
// its left sibling's subtree, i.e. the point emitted last (the same f64 value m, carried down
// unchanged), so a pending entry needs only (control, end): 4 doubles.
// These sequential walks are the EXCEPTION (see "Leaf-parallel flattening" below): one lane of a wave at a
// time runs them, on a work list in LDS (kMaxStack entries of 8 doubles per wave).  A private array would live
// in scratch memory: 1.2 KB per lane made the runtime set scratch up per dispatch and cost both flattening
// kernels ~25 us each, whatever they computed.
struct QuadStack {
	double *stk; // [kMaxStack][4]
	__device__ __forceinline__ void push(int n, double cx, double cy, double ex, double ey)
	{
		stk[4 * n + 0] = cx, stk[4 * n + 1] = cy, stk[4 * n + 2] = ex, stk[4 * n + 3] = ey;
	}
	__device__ __forceinline__ void pop(int n, double &cx, double &cy, double &ex, double &ey)
	{
		cx = stk[4 * n + 0], cy = stk[4 * n + 1], ex = stk[4 * n + 2], ey = stk[4 * n + 3];
	}
};
constexpr int kSerialStackDoubles = kMaxStack * 8;

// CAPPED = false is for curves whose subdivision provably ends within 16 levels (see flatten_quad_any): no
// bookkeeping in the loop.  CAPPED = true bounds the loop as described at kMaxCurvePoints.
template <bool CAPPED, class Emit>
__device__ __forceinline__ uint32_t flatten_quad(double sx, double sy, double cx, double cy, double ex, double ey,
                                                 double *stk, Emit emit)
{
	QuadStack st;
	st.stk = stk;
	int n = 0; // pending right halves = the reference's stack size after its pop
	uint32_t count = 0;
	double qsx = sx, qsy = sy, qcx = cx, qcy = cy, qex = ex, qey = ey;
	for (;;) {
		const double dx = qsx + qex - qcx * 2.0; // ring.rs:129
		const double dy = qsy + qey - qcy * 2.0;
		// (non-finite control points never become flat: the reference would not terminate;
		// here the work list is bounded and the end point is emitted)
		if (dx * dx + dy * dy <= kTolSq || (CAPPED && (n + 2 > kMaxStack || count >= kMaxCurvePoints))) {
			emit(qex, qey);
			count++;
			if (n == 0)
				break;
			qsx = qex, qsy = qey; // the right half starts where its left sibling ended
			n--;
			st.pop(n, qcx, qcy, qex, qey);
			continue;
		}
		const double m1x = (qsx + qcx) / 2.0, m1y = (qsy + qcy) / 2.0; // point.rs:29-31
		const double m2x = (qcx + qex) / 2.0, m2y = (qcy + qey) / 2.0;
		const double mx = (m1x + m2x) / 2.0, my = (m1y + m2y) / 2.0;
		st.push(n, m2x, m2y, qex, qey); // right half (m, m2, e): start implied
		n++;
		qcx = m1x, qcy = m1y, qex = mx, qey = my; // left half (s, m1, m)
	}
	return count;
}

// A quadratic's deviation s + e - 2c is quartered by every halving (exactly, up to roundings of the size of an ulp
// of the coordinates), so its square falls 16-fold per level: with the root's at most 0.01 * 16^14 and
// coordinates below 1e9 (ulp 1e-7, far below the tolerance) the loop ends within 16 levels and the work list
// never holds more than 16 entries — every curve of a real font.  Anything else takes the capped loop.
template <class Emit>
__device__ __forceinline__ uint32_t flatten_quad_any(double sx, double sy, double cx, double cy, double ex, double ey,
                                                     double *stk, Emit emit)
{
	const double dx = sx + ex - cx * 2.0, dy = sy + ey - cy * 2.0;
	const double m = fmax(fmax(fmax(fabs(sx), fabs(sy)), fmax(fabs(cx), fabs(cy))), fmax(fabs(ex), fabs(ey)));
	if (dx * dx + dy * dy <= 7.2e14 && m <= 1.0e9) // (false for NaN / inf)
		return flatten_quad<false>(sx, sy, cx, cy, ex, ey, stk, emit);
	return flatten_quad<true>(sx, sy, cx, cy, ex, ey, stk, emit);
}

// ring.rs:159-187
template <class Emit>
__device__ __forceinline__ uint32_t flatten_cubic(double sx, double sy, double ax, double ay, double bx, double by,
                                                  double ex, double ey, double *stk /*[kMaxStack][8], LDS*/, Emit emit)
{
	int n = 0;
	uint32_t count = 0;
	auto put = [&](int at, double v0, double v1, double v2, double v3, double v4, double v5, double v6, double v7) {
		double *e = stk + 8 * at;
		e[0] = v0, e[1] = v1, e[2] = v2, e[3] = v3, e[4] = v4, e[5] = v5, e[6] = v6, e[7] = v7;
	};
	put(n, sx, sy, ax, ay, bx, by, ex, ey);
	n++;
	while (n > 0) {
		n--;
		const double *t = stk + 8 * n;
		const double s0 = t[0], s1 = t[1], a0 = t[2], a1 = t[3], b0 = t[4], b1 = t[5], e0 = t[6], e1 = t[7];
		const double dx = (b0 + a0) - (s0 + e0);
		const double dy = (b1 + a1) - (s1 + e1);
		if (dx * dx + dy * dy <= kTolSq || n + 2 > kMaxStack || count >= kMaxCurvePoints) {
			emit(e0, e1);
			count++;
			continue;
		}
		const double p01x = (s0 + a0) / 2.0, p01y = (s1 + a1) / 2.0;
		const double p12x = (a0 + b0) / 2.0, p12y = (a1 + b1) / 2.0;
		const double p23x = (b0 + e0) / 2.0, p23y = (b1 + e1) / 2.0;
		const double p012x = (p01x + p12x) / 2.0, p012y = (p01y + p12y) / 2.0;
		const double p123x = (p12x + p23x) / 2.0, p123y = (p12y + p23y) / 2.0;
		const double mx = (p012x + p123x) / 2.0, my = (p012y + p123y) / 2.0;
		put(n, mx, my, p123x, p123y, p23x, p23y, e0, e1);
		n++;
		put(n, s0, s1, p01x, p01y, p012x, p012y, mx, my);
		n++;
	}
	return count;
}

// One command.  `ring_open` is false right after a CLOSE / at the glyph start, where the
// ring is empty and quad_to / curve_to are ignored (ring_builder.rs:83-85,99-101).
template <class Emit>
__device__ __forceinline__ uint32_t run_command(const OutlineCmd &c, bool ring_open, double lastx, double lasty, double *stk,
                                                Emit emit)
{
	switch (c.kind) {
	case CMD_MOVE: // ring_builder.rs:69-72 (save_ring happens in the ring pass)
	case CMD_LINE: // :75-77
		emit((double)c.x, (double)c.y);
		return 1;
	case CMD_QUAD: // :82-93
		if (!ring_open)
			return 0;
		return flatten_quad_any(lastx, lasty, (double)c.x1, (double)c.y1, (double)c.x, (double)c.y, stk, emit);
	case CMD_CURVE: // :98-110
		if (!ring_open)
			return 0;
		return flatten_cubic(lastx, lasty, (double)c.x1, (double)c.y1, (double)c.x2, (double)c.y2, (double)c.x, (double)c.y, stk, emit);
	default: // CMD_CLOSE
		return 0;
	}
}


// ring state in front of the 64 commands of one step of a wave: empty at the glyph start and after close();
// move_to and line_to make it non-empty; decided by the nearest earlier state-changing command (two ballots)
__device__ __forceinline__ bool ring_open_before(uint32_t kind, uint32_t lane, bool &carry)
{
	const unsigned long long opens = __ballot(kind == CMD_MOVE || kind == CMD_LINE);
	const unsigned long long closes = __ballot(kind == CMD_CLOSE);
	const unsigned long long before = (opens | closes) & ((1ull << lane) - 1ull);
	bool open = carry;
	if (before) {
		const int top = 63 - __builtin_clzll(before);
		open = (opens >> top) & 1ull;
	}
	const unsigned long long all = opens | closes;
	if (all) {
		const int top = 63 - __builtin_clzll(all);
		carry = (opens >> top) & 1ull;
	}
	return open;
}

// Rust `as i32` on f64: truncate, saturate, NaN -> 0
__device__ __forceinline__ int32_t to_i32(double v)
{
	if (v != v)
		return 0;
	if (v >= 2147483647.0)
		return 2147483647;
	if (v <= -2147483648.0)
		return (int32_t)0x80000000;
	return (int32_t)v;
}


// ---------------------------------------------------------------------------------------
// Leaf-parallel flattening of the 64 commands of a wave.
//
// The deviation s + e - 2c of a quadratic is quartered by every halving, exactly in real arithmetic: both halves
// of (s, c, e) have deviation (s + e - 2c) / 4.  So the reference's adaptive subdivision (ring.rs:119-144) is a
// COMPLETE binary tree of depth L = the first level with D / 16^L <= tolerance^2 (D = |s + e - 2c|^2 at the root),
// unless a rounding error pushes some node across the threshold.  The computed deviation of a node at level
// l <= 16 differs from d / 4^l by < (8 l + 8) 2^-52 M < 3e-14 M (every midpoint (a + b) / 2 rounds once, all
// points are convex combinations of the control points, |coordinate| <= M), so for M <= 1e6 the squared
// deviation near the threshold (|d| ~ 0.1) is off by < 6e-9 < 1e-6 * tolerance^2: when D / 16^L lies outside
// (1 +- 1e-6) tolerance^2 at levels L - 1 and L, the tree IS complete, the command appends exactly 2^L points
// and point r is the end point of the leaf reached from the root by the bits of r (most significant first) —
// the same midpoint operations on the same f64 values as the sequential walk, in any order.  (All 323 k
// quadratics of the 21 fixture fonts qualify; L is 4 or 5 for most.)
//
// A cubic's tree is adaptive, but its depth is bounded: with the second differences D1 = s - 2a + b, D2 = a - 2b + e
// the halves have (D1 / 4, (D1 + D2) / 8) and ((D1 + D2) / 8, D2 / 4), so M = max |component| of them falls at
// least 4-fold per level, and the reference's flatness measure (b + a) - (s + e) = -(D1 + D2) has a squared
// length <= 8 M^2: every node at depth Dmax = the first level with 16^Dmax >= 1.01 * 800 M0^2 is flat.  The
// 2^Dmax <= 64 "candidate" leaves of the complete tree of that depth are dealt out like a quadratic's points;
// the lane of a candidate item walks down from the root with the reference's own flatness test at every node
// and emits each adaptive leaf once, at the leaf's FIRST candidate.  A 64-bit mask of those first candidates per
// command (first flattening pass -> second) turns a candidate into the point's index: the number of mask bits
// below it.
//
// Everything else — a quadratic inside the margin, a cubic deeper than 6 levels, absurd coordinates, commands of a
// glyph whose transform is not monotone — keeps the sequential walk, one lane of the wave at a time.
//
// A wave therefore deals the points of its 64 commands out to its 64 lanes in ITEMS of up to 8 consecutive
// points (a subtree of depth <= 3; a line is an item of one point), 64 items per round: a curve of 32 points is
// four items and no longer keeps 63 lanes waiting, and the walk down to a subtree's root is shared by its 8 leaves.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kCubicFlag = 0x80000000u;
struct WaveQuads {
	double sx[64], sy[64], cx[64], cy[64], ex[64], ey[64]; // quadratic: s, c, e; cubic: s, a, e
	double bx[64], by[64];                                 // cubic: second control point
	uint32_t pre[65];             // exclusive sums of the commands' items
	uint32_t lev[64];             // depth of the (candidate) tree; kCubicFlag: cubic
	unsigned long long mask[64];  // cubic: first candidates of the adaptive leaves
};

struct CubicNode {
	double s0, s1, a0, a1, b0, b1, e0, e1;
};
__device__ __forceinline__ bool cubic_flat(const CubicNode &n)
{
	const double dx = (n.b0 + n.a0) - (n.s0 + n.e0); // ring.rs:171-172
	const double dy = (n.b1 + n.a1) - (n.s1 + n.e1);
	return dx * dx + dy * dy <= kTolSq;
}
__device__ __forceinline__ void cubic_split(const CubicNode &n, CubicNode &l, CubicNode &r)
{
	const double p01x = (n.s0 + n.a0) / 2.0, p01y = (n.s1 + n.a1) / 2.0; // ring.rs:176-182
	const double p12x = (n.a0 + n.b0) / 2.0, p12y = (n.a1 + n.b1) / 2.0;
	const double p23x = (n.b0 + n.e0) / 2.0, p23y = (n.b1 + n.e1) / 2.0;
	const double p012x = (p01x + p12x) / 2.0, p012y = (p01y + p12y) / 2.0;
	const double p123x = (p12x + p23x) / 2.0, p123y = (p12y + p23y) / 2.0;
	const double mx = (p012x + p123x) / 2.0, my = (p012y + p123y) / 2.0;
	l = CubicNode{n.s0, n.s1, p01x, p01y, p012x, p012y, mx, my};
	r = CubicNode{mx, my, p123x, p123y, p23x, p23y, n.e0, n.e1};
}
// depth bound of a cubic's adaptive tree (see above); false: not for the parallel rounds
__device__ __forceinline__ bool cubic_parallel_depth(const CubicNode &n, uint32_t &depth)
{
	const double d1x = n.s0 - 2.0 * n.a0 + n.b0, d1y = n.s1 - 2.0 * n.a1 + n.b1;
	const double d2x = n.a0 - 2.0 * n.b0 + n.e0, d2y = n.a1 - 2.0 * n.b1 + n.e1;
	const double M = fmax(fmax(fabs(d1x), fabs(d1y)), fmax(fabs(d2x), fabs(d2y)));
	const double m = fmax(fmax(fmax(fabs(n.s0), fabs(n.s1)), fmax(fabs(n.a0), fabs(n.a1))),
	                      fmax(fmax(fabs(n.b0), fabs(n.b1)), fmax(fabs(n.e0), fabs(n.e1))));
	depth = 0;
	if (!(M <= 1.0e6 && m <= 1.0e6)) // (false for NaN / inf)
		return false;
	const double need = 1.01 * 800.0 * M * M;
	double v = 1.0;
	uint32_t D = 0;
	while (v < need) {
		v *= 16.0;
		if (++D > 6)
			return false;
	}
	depth = D;
	return true;
}
// the adaptive leaves of the subtree under `n` that spans the candidates [c, c + 2^DL): emit(first candidate, end point)
template <int DL, class Emit>
__device__ __forceinline__ void cubic_subtree(const CubicNode &n, uint32_t c, bool &bound_broken, Emit &emit)
{
	if constexpr (DL == 0) {
		bound_broken |= !cubic_flat(n); // (cannot happen: the depth bound; the batch is refused if it does)
		emit(c, n.e0, n.e1);
	} else {
		if (cubic_flat(n)) {
			emit(c, n.e0, n.e1);
			return;
		}
		CubicNode l, r;
		cubic_split(n, l, r);
		cubic_subtree<DL - 1>(l, c, bound_broken, emit);
		cubic_subtree<DL - 1>(r, c + (1u << (DL - 1)), bound_broken, emit);
	}
}

// points this command hands to the parallel rounds (0: none or sequential), its tree depth
__device__ __forceinline__ uint32_t quad_parallel_points(double sx, double sy, double cx, double cy, double ex, double ey, uint32_t &lev)
{
	const double dx = sx + ex - cx * 2.0, dy = sy + ey - cy * 2.0; // ring.rs:129
	const double D = dx * dx + dy * dy;
	const double m = fmax(fmax(fmax(fabs(sx), fabs(sy)), fmax(fabs(cx), fabs(cy))), fmax(fabs(ex), fabs(ey)));
	lev = 0;
	if (!(D <= 7.2e14 && m <= 1.0e6)) // (false for NaN / inf)
		return 0;
	double v = D;
	uint32_t L = 0;
	while (v > kTolSq) { // <= 14 trips
		v *= 0.0625;
		L++;
	}
	const bool certain = v <= kTolSq * (1.0 - 1.0e-6) && (L == 0 || v * 16.0 > kTolSq * (1.0 + 1.0e-6));
	if (!certain)
		return 0;
	lev = L;
	return 1u << L;
}

// the complete subtree of depth D under (s, c, e), leaves in order: emit(end point of every leaf)
template <int D, class Emit>
__device__ __forceinline__ void quad_subtree(double sx, double sy, double cx, double cy, double ex, double ey, Emit &emit)
{
	if constexpr (D == 0) {
		emit(ex, ey);
	} else {
		const double m1x = (sx + cx) / 2.0, m1y = (sy + cy) / 2.0; // point.rs:29-31
		const double m2x = (cx + ex) / 2.0, m2y = (cy + ey) / 2.0;
		const double mx = (m1x + m2x) / 2.0, my = (m1y + m2y) / 2.0;
		quad_subtree<D - 1>(sx, sy, m1x, m1y, mx, my, emit); // left half (s, m1, m)
		quad_subtree<D - 1>(mx, my, m2x, m2y, ex, ey, emit); // right half (m, m2, e)
	}
}

constexpr uint32_t kItemDepth = 3; // an item = a subtree of up to 2^3 leaves

// The parallel rounds of one wave.  `n_items` / `lev` / control points: this lane's command (n_items = 0: it takes
// no part; for a cubic lev carries kCubicFlag and (cx, cy) / (bx, by) are its two control points).
// point(owner lane, index of the point inside its command, x, y) is called once per point of a line or quadratic,
// cubic_point(owner lane, first candidate of the leaf, x, y) once per leaf of a cubic, in order inside an item;
// done(owner lane) after the last point of an item.  Returns false if a cubic broke its depth bound.
template <class Point, class CubicPoint, class Done>
__device__ __forceinline__ bool wave_parallel_points(WaveQuads &w, uint32_t lane, uint32_t n_items, uint32_t lev, double sx, double sy,
                                                     double cx, double cy, double bx, double by, double ex, double ey, Point point,
                                                     CubicPoint cubic_point, Done done)
{
	uint32_t total;
	const uint32_t excl = wave_exclusive_sum(n_items, total);
	w.pre[lane] = excl;
	if (lane == 0)
		w.pre[64] = total;
	w.lev[lane] = lev;
	w.sx[lane] = sx, w.sy[lane] = sy, w.cx[lane] = cx, w.cy[lane] = cy, w.ex[lane] = ex, w.ey[lane] = ey;
	w.bx[lane] = bx, w.by[lane] = by;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	bool bound_broken = false;
	for (uint32_t q = lane; q < total; q += 64) {
		uint32_t k = 0; // the last command with pre[k] <= q (commands without items share their successor's offset)
#pragma unroll
		for (uint32_t step = 32; step > 0; step >>= 1)
			if (w.pre[k + step] <= q)
				k += step;
		const uint32_t lv = w.lev[k], L = lv & ~kCubicFlag, item = q - w.pre[k];
		const uint32_t Db = L < kItemDepth ? L : kItemDepth;
		if (lv & kCubicFlag) {
			CubicNode n{w.sx[k], w.sy[k], w.cx[k], w.cy[k], w.bx[k], w.by[k], w.ex[k], w.ey[k]};
			auto emit = [&](uint32_t c, double x, double y) { cubic_point(k, c, x, y); };
			bool in_item = true;
			// down to the item's root, the bits of `item` most significant first: an ancestor that is flat is a leaf
			// that spans this item and its neighbours; the first of them emits it
			for (uint32_t l = L - Db; l-- > 0;) {
				if (cubic_flat(n)) {
					if ((item & ((2u << l) - 1u)) == 0)
						emit(item << Db, n.e0, n.e1);
					in_item = false;
					break;
				}
				CubicNode lo, hi;
				cubic_split(n, lo, hi);
				n = ((item >> l) & 1u) ? hi : lo;
			}
			if (in_item) {
				const uint32_t c0 = item << Db;
				if (Db == 3)
					cubic_subtree<3>(n, c0, bound_broken, emit);
				else if (Db == 0)
					cubic_subtree<0>(n, c0, bound_broken, emit);
				else if (Db == 2)
					cubic_subtree<2>(n, c0, bound_broken, emit);
				else
					cubic_subtree<1>(n, c0, bound_broken, emit);
			}
			done(k);
			continue;
		}
		double qsx = w.sx[k], qsy = w.sy[k], qcx = w.cx[k], qcy = w.cy[k], qex = w.ex[k], qey = w.ey[k];
		// down to the item's root: the bits of `item`, most significant first
		for (uint32_t l = L - Db; l-- > 0;) {
			const double m1x = (qsx + qcx) / 2.0, m1y = (qsy + qcy) / 2.0; // point.rs:29-31
			const double m2x = (qcx + qex) / 2.0, m2y = (qcy + qey) / 2.0;
			const double mx = (m1x + m2x) / 2.0, my = (m1y + m2y) / 2.0;
			if ((item >> l) & 1u) { // right half (m, m2, e)
				qsx = mx, qsy = my, qcx = m2x, qcy = m2y;
			} else { // left half (s, m1, m)
				qcx = m1x, qcy = m1y, qex = mx, qey = my;
			}
		}
		uint32_t j = item << Db;
		auto emit = [&](double x, double y) {
			point(k, j, x, y);
			j++;
		};
		if (Db == 3)
			quad_subtree<3>(qsx, qsy, qcx, qcy, qex, qey, emit);
		else if (Db == 0)
			quad_subtree<0>(qsx, qsy, qcx, qcy, qex, qey, emit);
		else if (Db == 2)
			quad_subtree<2>(qsx, qsy, qcx, qcy, qex, qey, emit);
		else
			quad_subtree<1>(qsx, qsy, qcx, qcy, qex, qey, emit);
		done(k);
	}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	return !bound_broken;
}

// items a command of 2^depth points / candidates hands to the parallel rounds
__device__ __forceinline__ uint32_t items_of_depth(uint32_t depth) { return depth > kItemDepth ? 1u << (depth - kItemDepth) : 1u; }

// f64 <-> unsigned key with the same order (for integer atomics on LDS)
__device__ __forceinline__ unsigned long long f64_key(double v)
{
	const unsigned long long b = (unsigned long long)__double_as_longlong(v);
	return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_f64(unsigned long long k)
{
	return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// ---------------------------------------------------------------------------------------
// context: one wave per glyph.  Is the ring non-empty when command c arrives?  (quad_to / curve_to are ignored
// on an empty ring, ring_builder.rs:83-85,99-101.)
// ---------------------------------------------------------------------------------------
// PACKED: the commands arrive as one kind byte each plus only the coordinates their kind carries (move / line 2
// floats, quad 4, curve 6, close none: ~12 bytes per command of a TrueType font instead of 28 on the PCIe link);
// this pass also expands them into the OutlineCmd records every later pass reads (`cmds_out`).
template <bool PACKED>
__global__ __launch_bounds__(64) void outline_context(const OutlineCmd *__restrict__ cmds, const uint32_t *__restrict__ cmd_off,
                                                      const double *__restrict__ scale, uint32_t n_glyphs,
                                                      uint8_t *__restrict__ cmd_open, uint32_t *__restrict__ error_flag,
                                                      const uint8_t *__restrict__ kinds, const float *__restrict__ coords,
                                                      const uint32_t *__restrict__ dat_off, OutlineCmd *__restrict__ cmds_out)
{
	const uint32_t g = blockIdx.x, lane = threadIdx.x;
	if (g >= n_glyphs)
		return;
	const uint32_t c0 = cmd_off[g], c1 = cmd_off[g + 1];
	const double sc = scale[g];
	// bit 1: the glyph's transform is not monotone increasing (scale <= 0 or not finite): the count pass then takes
	// the bounding boxes on the transformed points
	const uint8_t odd = (sc > 0.0 && sc < __builtin_huge_val()) ? 0 : 2;
	bool carry = false;
	uint32_t d_at = 0, d_end = 0; // this glyph's coordinates: coords[d_at, d_end)
	if constexpr (PACKED) {
		d_at = dat_off[g];
		d_end = dat_off[g + 1];
	}
	for (uint32_t base = c0; base < c1; base += 64) {
		const uint32_t c = base + lane;
		uint32_t k = 0xFFu;
		if constexpr (PACKED) {
			if (c < c1)
				k = kinds[c];
			const uint32_t nf = k <= CMD_LINE ? 2u : (k == CMD_QUAD ? 4u : (k == CMD_CURVE ? 6u : 0u));
			uint32_t total;
			const uint32_t at = d_at + wave_exclusive_sum(nf, total);
			d_at += total;
			if (c < c1) {
				OutlineCmd o;
				o.x1 = o.y1 = o.x2 = o.y2 = o.x = o.y = 0.0f;
				o.kind = k;
				if (at + nf > d_end) { // the offsets do not match the kinds: nothing is read past the glyph's range
					atomicOr(error_flag, 8u);
					o.kind = CMD_CLOSE;
					k = CMD_CLOSE;
				} else if (nf == 2) {
					o.x = coords[at], o.y = coords[at + 1];
				} else if (nf == 4) {
					o.x1 = coords[at], o.y1 = coords[at + 1], o.x = coords[at + 2], o.y = coords[at + 3];
				} else if (nf == 6) {
					o.x1 = coords[at], o.y1 = coords[at + 1], o.x2 = coords[at + 2], o.y2 = coords[at + 3];
					o.x = coords[at + 4], o.y = coords[at + 5];
				}
				cmds_out[c] = o;
			}
		} else {
			k = c < c1 ? cmds[c].kind : 0xFFu;
		}
		const bool open = ring_open_before(k, lane, carry);
		if (c < c1) {
			cmd_open[c] = (uint8_t)((open ? 1 : 0) | odd);
			if (k > CMD_CLOSE) // not one of the five callbacks: every kernel treats it as a no-op, the batch is refused
				atomicOr(error_flag, 2u);
		}
	}
}

constexpr int kFlattenThreads = 64; // one wave per workgroup

// ---------------------------------------------------------------------------------------
// count: thread per command — the first flattening pass (ring.rs:119-187).  Stores the number of points the
// command appends and the bounding box of those points: of the raw points when the glyph's transform is
// monotone (scale > 0: the ring pass transforms four numbers instead of every point), else of the
// transformed points (point.rs:96-99, 83-86).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFlattenThreads) void outline_count(const OutlineCmd *__restrict__ cmds,
                                                                 const uint8_t *__restrict__ cmd_open, uint32_t n_cmds,
                                                                 const uint32_t *__restrict__ cmd_off, uint32_t n_glyphs,
                                                                 const double *__restrict__ scale,
                                                                 const double *__restrict__ shift_x,
                                                                 uint32_t *__restrict__ counts, double4 *__restrict__ cmd_box,
                                                                 unsigned long long *__restrict__ cmd_mask,
                                                                 uint32_t *__restrict__ error_flag)
{
	__shared__ double s_stack[kSerialStackDoubles];
	__shared__ WaveQuads s_w;
	__shared__ unsigned long long s_box[4][64]; // per command: min x, min y (keys), max x, max y
	const uint32_t lane = threadIdx.x;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool valid = i < n_cmds;
	OutlineCmd cmd;
	cmd.kind = CMD_CLOSE;
	cmd.x = cmd.y = cmd.x1 = cmd.y1 = cmd.x2 = cmd.y2 = 0.0f;
	uint8_t ctx = 0;
	if (valid) {
		cmd = cmds[i];
		ctx = cmd_open[i];
	}
	const bool open = (ctx & 1) != 0;
	// when the ring is open the previous command of the glyph emitted at least one point and ended on its own
	// (x, y): that is the current point of the ring
	const double lx = open ? (double)cmds[i - 1].x : 0.0, ly = open ? (double)cmds[i - 1].y : 0.0;
	const double inf = __builtin_huge_val();
	const bool raw_boxes = (ctx & 2) == 0;
	// parallel rounds: move_to / line_to (one point, a tree of depth 0), the quadratics with a complete tree, the
	// cubics with a depth bound of at most 6
	uint32_t n_par = 0, n_items = 0, lev = 0;
	bool cubic = false;
	if (valid && raw_boxes) {
		if (cmd.kind == CMD_MOVE || cmd.kind == CMD_LINE) {
			n_par = n_items = 1;
		} else if (cmd.kind == CMD_QUAD && open) {
			n_par = quad_parallel_points(lx, ly, (double)cmd.x1, (double)cmd.y1, (double)cmd.x, (double)cmd.y, lev);
			n_items = n_par ? items_of_depth(lev) : 0u;
		} else if (cmd.kind == CMD_CURVE && open) {
			const CubicNode root{lx, ly, (double)cmd.x1, (double)cmd.y1, (double)cmd.x2, (double)cmd.y2, (double)cmd.x, (double)cmd.y};
			cubic = cubic_parallel_depth(root, lev);
			if (cubic) {
				n_items = items_of_depth(lev);
				lev |= kCubicFlag;
			}
		}
	}
	s_box[0][lane] = s_box[1][lane] = f64_key(inf);
	s_box[2][lane] = s_box[3][lane] = f64_key(-inf);
	s_w.mask[lane] = 0;
	{
		double bx0 = inf, by0 = inf, bx1 = -inf, by1 = -inf; // box of the item being walked
		unsigned long long leaves = 0;                        // first candidates of the cubic leaves of the item
		auto grow = [&](double x, double y) {
			bx0 = fmin(bx0, x); // bbox.rs:64-69 (fmin / fmax skip NaN)
			by0 = fmin(by0, y);
			bx1 = fmax(bx1, x);
			by1 = fmax(by1, y);
		};
		const bool ok = wave_parallel_points(
		    s_w, lane, n_items, lev, lx, ly, (double)cmd.x1, (double)cmd.y1, (double)cmd.x2, (double)cmd.y2, (double)cmd.x, (double)cmd.y,
		    [&](uint32_t, uint32_t, double x, double y) { grow(x, y); },
		    [&](uint32_t, uint32_t c, double x, double y) {
			    grow(x, y);
			    leaves |= 1ull << c;
		    },
		    [&](uint32_t k) {
			    atomicMin(&s_box[0][k], f64_key(bx0));
			    atomicMin(&s_box[1][k], f64_key(by0));
			    atomicMax(&s_box[2][k], f64_key(bx1));
			    atomicMax(&s_box[3][k], f64_key(by1));
			    if (leaves)
				    atomicOr(&s_w.mask[k], leaves);
			    bx0 = inf, by0 = inf, bx1 = -inf, by1 = -inf;
			    leaves = 0;
		    });
		if (!ok)
			atomicOr(error_flag, 4u); // (a cubic deeper than its bound: never seen; the batch is refused rather than wrong)
	}
	if (cubic) {
		n_par = (uint32_t)__builtin_popcountll(s_w.mask[lane]);
		cmd_mask[i] = s_w.mask[lane];
	}
	if (valid && n_items != 0) {
		counts[i] = n_par;
		cmd_box[i] = make_double4(key_f64(s_box[0][lane]), key_f64(s_box[1][lane]), key_f64(s_box[2][lane]), key_f64(s_box[3][lane]));
	}
	// sequential walks, one lane at a time (they share the wave's work list in LDS); quad_to / curve_to on an empty
	// ring and close() append nothing and need no walk
	const bool walk = valid && n_items == 0 && (cmd.kind == CMD_MOVE || cmd.kind == CMD_LINE || ((cmd.kind == CMD_QUAD || cmd.kind == CMD_CURVE) && open));
	if (valid && n_items == 0 && !walk) {
		counts[i] = 0;
		cmd_box[i] = make_double4(inf, inf, -inf, -inf);
	}
	for (unsigned long long todo = __ballot(walk); todo; todo &= todo - 1) {
		if (lane != (uint32_t)__builtin_ctzll(todo))
			continue;
		double minx = inf, miny = inf, maxx = -inf, maxy = -inf;
		double sc = 1.0, dx = 0.0;
		if (!raw_boxes) { // rare: find the glyph (last g with cmd_off[g] <= i) for its scale and shift
			uint32_t lo = 0, hi = n_glyphs;
			while (hi - lo > 1) {
				const uint32_t mid = (lo + hi) >> 1;
				if (cmd_off[mid] <= i)
					lo = mid;
				else
					hi = mid;
			}
			sc = scale[lo];
			dx = shift_x[lo];
		}
		counts[i] = run_command(cmd, open, lx, ly, s_stack, [&](double x, double y) {
			if (!raw_boxes) {
				x *= sc;
				y *= sc;
				x += dx;
				y += 0.0;
			}
			minx = fmin(minx, x); // bbox.rs:64-69 (fmin / fmax skip NaN)
			miny = fmin(miny, y);
			maxx = fmax(maxx, x);
			maxy = fmax(maxy, y);
		});
		cmd_box[i] = make_double4(minx, miny, maxx, maxy);
	}
}

// ---------------------------------------------------------------------------------------
// rings: one wave per glyph, lane <-> command, no serial walk:
//   pass 1: exclusive sums of the commands' point counts = every command's first point inside the glyph.
//   pass 2: RingBuilder::save_ring + Ring::close (ring_builder.rs:33-54, ring.rs:53-63).  With `open` = the ring
//     is non-empty in front of a command (context pass): a command STARTS a ring if it is a move_to, or a
//     line_to on an empty ring (ring_builder.rs:69-77); it ENDS the ring collected so far if that ring is open
//     and the command is a move_to or a close (save_ring); the glyph's end saves the last open ring
//     (into_rings, :26-29).  The lane of the ending command writes the ring's record.  A ring's first point is
//     the point of the command that opened it and its last point is the end point of its last command (every
//     command inside an open ring ends on its own (x, y)), so the rules need no stored points.
//   pass 3: bbox of the accepted rings' points = union of their commands' boxes pushed through the transform
//     (scale > 0 and the shift are monotone; for any other scale the count pass took the boxes on the
//     transformed points), then Renderer::prepare_glyph (renderer.rs:64-91, 122-137).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void outline_rings(const OutlineCmd *__restrict__ cmds, const uint32_t *__restrict__ cmd_off,
                                                    const uint8_t *__restrict__ cmd_open, const double *__restrict__ scale,
                                                    const double *__restrict__ shift_x, uint32_t n_glyphs,
                                                    const uint32_t *__restrict__ counts, uint32_t *__restrict__ pt_local,
                                                    const double4 *__restrict__ cmd_box, RingRec *__restrict__ rings,
                                                    uint32_t *__restrict__ cmd_ring, OutlineRect *__restrict__ rects,
                                                    uint32_t *__restrict__ error_flag)
{
	const uint32_t g = blockIdx.x, lane = threadIdx.x;
	if (g >= n_glyphs)
		return;
	const uint32_t c0 = cmd_off[g], c1 = cmd_off[g + 1];
	const double sc = scale[g], dx = shift_x[g];
	const double inf = __builtin_huge_val();
	const bool raw_boxes = sc > 0.0 && sc < inf; // (the count pass made the same decision)
	// What the passes hand each other (point offsets, ring of a command, ring accepted) also stays in LDS for glyphs
	// of up to kRingsLds commands (every glyph of the fixture fonts): no round trip through memory between the passes
	constexpr uint32_t kRingsLds = 1024;
	__shared__ uint32_t s_pt[kRingsLds + 1], s_ring[kRingsLds];
	__shared__ uint8_t s_acc[kRingsLds];
	const bool in_lds = c1 - c0 <= kRingsLds;
	auto pt_at = [&](uint32_t c) { return in_lds ? s_pt[c - c0] : pt_local[c + g]; }; // c in [c0, c1]

	// ---- pass 1 ----
	uint32_t pbase = 0;
	unsigned long long total64 = 0;
	for (uint32_t base = c0; base < c1; base += 64) {
		const uint32_t c = base + lane;
		const bool valid = c < c1;
		const uint32_t cnt = valid ? counts[c] : 0u;
		uint32_t total;
		const uint32_t excl = wave_exclusive_sum(cnt, total);
		if (valid) {
			pt_local[c + g] = pbase + excl; // (one slot per command plus one end slot per glyph)
			if (in_lds)
				s_pt[c - c0] = pbase + excl;
		}
		pbase += total;
		total64 += total;
	}
	if (lane == 0) {
		pt_local[c1 + g] = pbase;
		if (in_lds)
			s_pt[c1 - c0] = pbase;
		if (total64 > (1ull << 28)) // (also keeps the 32-bit point offsets of a glyph exact)
			atomicOr(error_flag, 1u);
	}
	__syncthreads(); // pt_local is read back below (other lanes' entries)

	// ---- pass 2 ----
	auto ring_rec = [&](uint32_t ra, uint32_t rb) {
		RingRec r;
		const uint32_t a = pt_at(ra), b = pt_at(rb); // points [a, b) of the glyph
		r.pt_first = a;
		r.pt_count = b - a;
		r.append = 0;
		r.accepted = 0;
		r.seg_local = 0;
		r.glyph = g;
		if (r.pt_count >= 3) { // ring_builder.rs:35-38
			const double fx = (double)cmds[ra].x, fy = (double)cmds[ra].y, lx = (double)cmds[rb - 1].x, ly = (double)cmds[rb - 1].y;
			const double eps = 2.220446049250313e-16;
			r.append = (fabs(fx - lx) > eps || fabs(fy - ly) > eps) ? 1u : 0u; // ring.rs:60-62
			if (r.pt_count + r.append >= 4)                                      // ring_builder.rs:45-48
				r.accepted = 1;
		}
		return r;
	};
	uint32_t last_start = 0xFFFFFFFFu; // the command that opened the ring being collected (wave-uniform carry)
	bool open_after = false;          // ring non-empty behind the last command seen
	uint32_t seg_base = 0, n_rings_acc = 0;
	for (uint32_t base = c0; base < c1; base += 64) {
		const uint32_t c = base + lane;
		const bool valid = c < c1;
		const uint32_t k = valid ? cmds[c].kind : 0xFFu;
		const bool open = valid && (cmd_open[c] & 1);
		const bool starts = k == CMD_MOVE || (k == CMD_LINE && !open);
		const bool ends_cmd = open && (k == CMD_MOVE || k == CMD_CLOSE);
		const bool have_after = k == CMD_MOVE || k == CMD_LINE || (valid && k != CMD_CLOSE && open);
		// nearest ring start at or before this lane (strictly before for the ring this command ends)
		const unsigned long long sb = __ballot(starts);
		const unsigned long long below = sb & ((1ull << lane) - 1ull);
		const uint32_t start_before = below ? base + (uint32_t)(63 - __builtin_clzll(below)) : last_start;
		const uint32_t start_here = starts ? c : start_before;
		// (an "open" ring has a command that opened it — context bytes that say otherwise would index ring 0xFFFFFFFF)
		const bool ends = ends_cmd && start_before != 0xFFFFFFFFu;
		if (valid) {
			cmd_ring[c] = have_after ? start_here : 0xFFFFFFFFu;
			if (in_lds)
				s_ring[c - c0] = have_after ? start_here : 0xFFFFFFFFu;
		}
		RingRec rec;
		rec.accepted = 0;
		uint32_t segs = 0;
		if (ends) {
			rec = ring_rec(start_before, c);
			if (rec.accepted)
				segs = rec.pt_count + rec.append - 1;
		}
		uint32_t tot_segs, tot_acc;
		const uint32_t seg_excl = wave_exclusive_sum(segs, tot_segs);
		(void)wave_exclusive_sum(ends ? rec.accepted : 0u, tot_acc);
		if (ends) {
			rec.seg_local = seg_base + seg_excl;
			rings[start_before] = rec; // ring records live at the index of the command that opened them
			if (in_lds)
				s_acc[start_before - c0] = (uint8_t)rec.accepted;
		}
		seg_base += tot_segs;
		n_rings_acc += tot_acc;
		if (sb)
			last_start = base + (uint32_t)(63 - __builtin_clzll(sb));
		const unsigned long long ha = __ballot(have_after);
		const uint32_t n_valid = min(64u, c1 - base);
		open_after = (ha >> (n_valid - 1)) & 1ull;
	}
	if (open_after && lane == 0 && last_start != 0xFFFFFFFFu) { // into_rings: the ring still open at the end of the glyph
		RingRec rec = ring_rec(last_start, c1);
		rec.seg_local = seg_base;
		if (rec.accepted) {
			seg_base += rec.pt_count + rec.append - 1;
			n_rings_acc++;
		}
		rings[last_start] = rec;
		if (in_lds)
			s_acc[last_start - c0] = (uint8_t)rec.accepted;
	}
	seg_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg_base);
	n_rings_acc = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_rings_acc);
	__syncthreads(); // cmd_ring / rings are read back below

	// ---- pass 3 ----
	double minx = inf, miny = inf, maxx = -inf, maxy = -inf;
	for (uint32_t c = c0 + lane; c < c1; c += 64) {
		const uint32_t rs = in_lds ? s_ring[c - c0] : cmd_ring[c];
		if (rs != 0xFFFFFFFFu && (in_lds ? s_acc[rs - c0] != 0 : rings[rs].accepted != 0)) {
			const double4 bx = cmd_box[c];
			minx = fmin(minx, bx.x);
			miny = fmin(miny, bx.y);
			maxx = fmax(maxx, bx.z);
			maxy = fmax(maxy, bx.w);
		}
	}
	if (raw_boxes) {
		minx *= sc, miny *= sc, maxx *= sc, maxy *= sc; // point.rs:96-99
		minx += dx, maxx += dx;                         // point.rs:83-86
		miny += 0.0, maxy += 0.0;
	}
	for (int sh = 32; sh > 0; sh >>= 1) { // fmin/fmax are exact selections: any order gives the same box
		minx = fmin(minx, __shfl_xor(minx, sh));
		miny = fmin(miny, __shfl_xor(miny, sh));
		maxx = fmax(maxx, __shfl_xor(maxx, sh));
		maxy = fmax(maxy, __shfl_xor(maxy, sh));
	}
	if (lane == 0) {
		const uint32_t nseg = seg_base, n_rings = n_rings_acc;
		OutlineRect rc;
		rc.x0 = rc.y0 = 0;
		rc.w = rc.h = 0;
		rc.n_segments = 0;
		rc.has_raster = 0;
		// renderer.rs:118-120 (no rings) and :133-137 / bbox.rs:56-58 (empty bbox) -> PbfGlyph::empty
		if (n_rings > 0 && !(maxx <= minx && maxy <= miny)) {
			const int32_t x0 = to_i32(floor(minx)) - 3, y0 = to_i32(floor(miny)) - 3; // renderer.rs:73-76, BUFFER = 3
			const int32_t x1 = to_i32(ceil(maxx)) + 3, y1 = to_i32(ceil(maxy)) + 3;
			rc.x0 = x0;
			rc.y0 = y0;
			rc.w = (uint32_t)(x1 - x0);
			rc.h = (uint32_t)(y1 - y0);
			rc.n_segments = nseg;
			rc.has_raster = 1;
		}
		rects[g] = rc;
	}
}

// ---------------------------------------------------------------------------------------
// chunk boxes from the commands' boxes (one wave per glyph of more than two chunks).  The raster skips a chunk of 256
// segments whose box is far from a span (sdf_span_kernel.inc); sdf_chunk_boxes takes those boxes from the segments, i.e.
// behind the second flattening pass, on the path every bitmap waits for.  Everything needed for a box that CONTAINS the
// chunk's segments is known once the plan has run: the count pass stored the box of the points every command appends, the
// ring pass where those points sit in their ring, the plan where the glyph's segments start.  Point q of an accepted ring
// (ring-local) starts segment q and ends segment q - 1; with the appended copy of point 0 (Ring::close, ring.rs:53-63)
// point 0 also ends the ring's last segment.  So a command whose points are [qa, qb) touches the ring's segments
// max(qa - 1, 0) .. min(qb - 1, last), plus the last one if it holds point 0 of a closed-by-append ring: its box goes into
// the chunks of those segments.  Both end points of every segment are covered that way, so the union is a superset of the
// exact box (by a command's extent, a few dozen points): chunks are skipped a little less often, never wrongly.  Boxes are
// pushed through the glyph's transform exactly as the ring pass does (monotone for scale > 0; for any other scale the count
// pass took them on the transformed points), then made relative to (x0, y0) and rounded to f32 like sdf_chunk_boxes' — the
// raster's pad covers the rounding.  The first `n_box_glyphs` workgroups of outline_emit_segments' grid do this, one glyph each,
// beside the second flattening pass: no launch and no dependency of its own (a separate stream for it cost what it saved).
// ---------------------------------------------------------------------------------------
constexpr uint32_t kBoxLdsChunks = 256; // glyphs of more chunks (> 65 536 segments) get boxes that contain everything

__device__ __forceinline__ void chunk_boxes_of_glyph(uint32_t g, uint32_t lane, uint32_t (*s_key)[kBoxLdsChunks] /* [4]: min x, min y, max x, max y
                                                     as order-preserving keys of the f32 values */,
                                                     const uint32_t *__restrict__ cmd_off, const double *__restrict__ scale,
                                                     const double *__restrict__ shift_x, const uint32_t *__restrict__ pt_local,
                                                     const RingRec *__restrict__ rings, const uint32_t *__restrict__ cmd_ring,
                                                     const double4 *__restrict__ cmd_box, const GlyphDesc *__restrict__ descs,
                                                     float4 *__restrict__ boxes)
{
	const GlyphDesc d = descs[g];
	if (d.n_seg <= 2u * 256u) // (the raster asks for boxes only when a glyph has more than two chunks)
		return;
	const uint32_t n_chunks = (d.n_seg + 255u) >> 8;
	const float inf = __builtin_inff();
	if (n_chunks > kBoxLdsChunks) {
		for (uint32_t c = lane; c < n_chunks; c += 64u)
			boxes[chunk_box_index(d.seg_off, g, c)] = make_float4(-inf, -inf, inf, inf);
		return;
	}
	auto key = [](float v) { // f32 -> u32 with the same order
		const uint32_t b = __float_as_uint(v);
		return (b >> 31) ? ~b : (b | 0x80000000u);
	};
	auto unkey = [](uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); };
	for (uint32_t c = lane; c < n_chunks; c += 64u) {
		s_key[0][c] = s_key[1][c] = key(inf);
		s_key[2][c] = s_key[3][c] = key(-inf);
	}
	__syncthreads();
	const uint32_t c0 = cmd_off[g], c1 = cmd_off[g + 1];
	const double sc = scale[g], dx = shift_x[g];
	const bool raw_boxes = sc > 0.0 && sc < __builtin_huge_val(); // (as the count and ring passes decide)
	for (uint32_t c = c0 + lane; c < c1; c += 64u) {
		const uint32_t rs = cmd_ring[c];
		if (rs == 0xFFFFFFFFu)
			continue;
		const RingRec r = rings[rs];
		const uint32_t a = pt_local[c + g], b = pt_local[c + 1 + g]; // the command's points inside the glyph
		if (!r.accepted || b <= a || a < r.pt_first)
			continue;
		const uint32_t last = r.pt_count + r.append - 2u; // last segment of the ring (accepted: pt_count + append >= 4)
		const uint32_t qa = a - r.pt_first, qb = b - r.pt_first;
		const uint32_t s_lo = qa ? qa - 1u : 0u, s_hi = min(qb - 1u, last);
		double4 bx = cmd_box[c];
		if (raw_boxes) {
			bx.x *= sc, bx.y *= sc, bx.z *= sc, bx.w *= sc; // point.rs:96-99
			bx.x += dx, bx.z += dx;                         // point.rs:83-86
			bx.y += 0.0, bx.w += 0.0;
		}
		float x0 = (float)(bx.x - (double)d.x0), y0 = (float)(bx.y - (double)d.y0);
		float x1 = (float)(bx.z - (double)d.x0), y1 = (float)(bx.w - (double)d.y0);
		if (!(fabsf(x0) < 3.0e38f) || !(fabsf(y0) < 3.0e38f) || !(fabsf(x1) < 3.0e38f) || !(fabsf(y1) < 3.0e38f))
			x0 = y0 = -inf, x1 = y1 = inf; // non-finite: the chunks it touches are never skipped
		auto put = [&](uint32_t s_first, uint32_t s_last) {
			const uint32_t k_lo = (r.seg_local + s_first) >> 8, k_hi = min((r.seg_local + s_last) >> 8, n_chunks - 1u);
			for (uint32_t k = k_lo; k <= k_hi; k++) {
				atomicMin(&s_key[0][k], key(x0));
				atomicMin(&s_key[1][k], key(y0));
				atomicMax(&s_key[2][k], key(x1));
				atomicMax(&s_key[3][k], key(y1));
			}
		};
		if (s_lo <= s_hi)
			put(s_lo, s_hi);
		if (qa == 0u && r.append)
			put(last, last); // point 0 ends the segment Ring::close appended
	}
	__syncthreads();
	for (uint32_t c = lane; c < n_chunks; c += 64u) {
		float4 o = make_float4(unkey(s_key[0][c]), unkey(s_key[1][c]), unkey(s_key[2][c]), unkey(s_key[3][c]));
		if (!(o.x <= o.z) || !(o.y <= o.w)) // nothing arrived (cannot happen: every segment has end points): never skip
			o = make_float4(-inf, -inf, inf, inf);
		boxes[chunk_box_index(d.seg_off, g, c)] = o;
	}
}

// ---------------------------------------------------------------------------------------
// emit: thread per command — the second flattening pass.  Point i of a ring of n points is the start of segment i
// (i <= n - 2, or i == n - 1 when Ring::close appended the first point again) and the end of segment i - 1; with
// the appended point, point 0 also ends segment n - 1 (Rings::get_segments, rings.rs:75-81) — written straight
// into the segment records {sx, sy, ex, ey} after scale + translate (renderer.rs:122-131); the raster reads
// them with a stride of four doubles.  A command that belongs to a ring has the
// ring open in front of it unless it opened the ring itself (move_to / line_to, which do not care).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFlattenThreads) void outline_emit_segments(const OutlineCmd *__restrict__ cmds, uint32_t n_cmds,
                                                                         const uint8_t *__restrict__ cmd_open,
                                                                         const double *__restrict__ scale,
                                                                         const double *__restrict__ shift_x,
                                                                         const uint32_t *__restrict__ pt_local,
                                                                         const RingRec *__restrict__ rings,
                                                                         const uint32_t *__restrict__ cmd_ring,
                                                                         const GlyphDesc *__restrict__ descs,
                                                                         const PlanHeader *__restrict__ hdr,
                                                                         unsigned long long seg_cap, double2 *__restrict__ seg,
                                                                         const unsigned long long *__restrict__ cmd_mask,
                                                                         uint32_t n_box_glyphs, const uint32_t *__restrict__ cmd_off,
                                                                         const double4 *__restrict__ cmd_box, float4 *__restrict__ boxes)
{
	__shared__ double s_stack[kSerialStackDoubles];
	__shared__ WaveQuads s_w;
	__shared__ uint32_t s_key[4][kBoxLdsChunks];
	// per command, for the lanes that place its points: first record of its ring, index of its first point inside
	// the ring, the ring's point count and closing flag, the glyph's transform
	__shared__ unsigned long long s_seg0[64];
	__shared__ uint32_t s_idx0[64], s_n[64], s_append[64];
	__shared__ double s_sc[64], s_dx[64];
	if (hdr->error || hdr->n_segments > seg_cap) // nothing may be written: the host grows the arrays and launches again
		return;
	const uint32_t lane = threadIdx.x;
	// the first n_box_glyphs workgroups: chunk boxes of one glyph each (see chunk_boxes_of_glyph), first so that the longest
	// of them are under way when the flattening workgroups fill the chip
	if (blockIdx.x < n_box_glyphs) {
		chunk_boxes_of_glyph(blockIdx.x, lane, s_key, cmd_off, scale, shift_x, pt_local, rings, cmd_ring, cmd_box, descs, boxes);
		return;
	}
	const uint32_t c = (blockIdx.x - n_box_glyphs) * blockDim.x + threadIdx.x;
	bool active = c < n_cmds;
	uint32_t rcmd = 0xFFFFFFFFu;
	RingRec r;
	r.accepted = 0, r.append = 0, r.pt_count = 0, r.pt_first = 0, r.seg_local = 0, r.glyph = 0;
	GlyphDesc d;
	d.n_seg = 0, d.seg_off = 0;
	if (active) {
		rcmd = cmd_ring[c];
		active = rcmd != 0xFFFFFFFFu;
	}
	if (active) {
		r = rings[rcmd];
		active = r.accepted != 0;
	}
	if (active) {
		d = descs[r.glyph];
		active = d.n_seg != 0; // else PbfGlyph::empty (empty bbox): nothing is rasterised
	}
	OutlineCmd cmd;
	cmd.kind = CMD_CLOSE;
	cmd.x = cmd.y = cmd.x1 = cmd.y1 = cmd.x2 = cmd.y2 = 0.0f;
	double sc = 1.0, dx = 0.0;
	uint32_t idx = 0;
	bool monotone = false;
	if (active) {
		cmd = cmds[c];
		sc = scale[r.glyph], dx = shift_x[r.glyph];
		idx = pt_local[c + r.glyph] - r.pt_first; // position of the command's first point inside its ring
		monotone = (cmd_open[c] & 2) == 0;       // (the count pass took the sequential walk for the other glyphs)
	}
	const bool open = active && c != rcmd;
	const double lx = open ? (double)cmds[c - 1].x : 0.0, ly = open ? (double)cmds[c - 1].y : 0.0;
	const size_t seg0 = (size_t)d.seg_off + r.seg_local;
	// point `at` of a ring of n points (scaled + shifted): start of segment `at`, end of segment `at - 1`
	auto place = [&](size_t base, uint32_t at, uint32_t n, uint32_t append, double x, double y) {
		// records {sx, sy, ex, ey}: two 16-byte stores per point, side by side in memory
		if (at + 1 < n || append) // start of segment at
			seg[2 * (base + at)] = make_double2(x, y);
		if (at >= 1) // end of segment at - 1
			seg[2 * (base + at - 1) + 1] = make_double2(x, y);
		else if (append) // the closing segment (n - 1) returns to the first point
			seg[2 * (base + n - 1) + 1] = make_double2(x, y);
	};
	uint32_t n_items = 0, lev = 0;
	unsigned long long mask = 0;
	if (active && monotone) { // the same split as in the count pass
		if (cmd.kind == CMD_MOVE || cmd.kind == CMD_LINE) {
			n_items = 1;
		} else if (cmd.kind == CMD_QUAD && open) {
			if (quad_parallel_points(lx, ly, (double)cmd.x1, (double)cmd.y1, (double)cmd.x, (double)cmd.y, lev))
				n_items = items_of_depth(lev);
		} else if (cmd.kind == CMD_CURVE && open) {
			const CubicNode root{lx, ly, (double)cmd.x1, (double)cmd.y1, (double)cmd.x2, (double)cmd.y2, (double)cmd.x, (double)cmd.y};
			if (cubic_parallel_depth(root, lev)) {
				n_items = items_of_depth(lev);
				lev |= kCubicFlag;
				mask = cmd_mask[c]; // first candidates of the leaves, from the count pass
			}
		}
	}
	s_seg0[lane] = (unsigned long long)seg0;
	s_idx0[lane] = idx;
	s_n[lane] = r.pt_count;
	s_append[lane] = r.append;
	s_sc[lane] = sc;
	s_dx[lane] = dx;
	s_w.mask[lane] = mask;
	auto put = [&](uint32_t k, uint32_t j, double x, double y) {
		const double ksc = s_sc[k];
		x *= ksc; // point.rs:96-99
		y *= ksc;
		x += s_dx[k]; // point.rs:83-86
		y += 0.0;
		place((size_t)s_seg0[k], s_idx0[k] + j, s_n[k], s_append[k], x, y);
	};
	(void)wave_parallel_points(
	    s_w, lane, n_items, lev, lx, ly, (double)cmd.x1, (double)cmd.y1, (double)cmd.x2, (double)cmd.y2, (double)cmd.x, (double)cmd.y,
	    [&](uint32_t k, uint32_t j, double x, double y) { put(k, j, x, y); },
	    [&](uint32_t k, uint32_t cand, double x, double y) {
		    // the leaf's index inside its command: the leaves in front of it
		    put(k, (uint32_t)__builtin_popcountll(s_w.mask[k] & ((1ull << cand) - 1ull)), x, y);
	    },
	    [](uint32_t) {});
	// sequential walks, one lane at a time (they share the wave's work list in LDS)
	const bool walk = active && n_items == 0 && (cmd.kind == CMD_MOVE || cmd.kind == CMD_LINE || ((cmd.kind == CMD_QUAD || cmd.kind == CMD_CURVE) && open));
	for (unsigned long long todo = __ballot(walk); todo; todo &= todo - 1) {
		if (lane != (uint32_t)__builtin_ctzll(todo))
			continue;
		run_command(cmd, open, lx, ly, s_stack, [&](double x, double y) {
			x *= sc; // point.rs:96-99
			y *= sc;
			x += dx; // point.rs:83-86
			y += 0.0;
			place(seg0, idx, r.pt_count, r.append, x, y);
			idx++;
		});
	}
}

} // namespace vgsdf

using namespace vgsdf;

extern "C" int vgsdf_outline_context(const OutlineCmd *cmds, const uint32_t *cmd_off, const double *scale, uint32_t n_glyphs,
                                     uint8_t *cmd_open, uint32_t *error_flag, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	hipLaunchKernelGGL(outline_context<false>, dim3(n_glyphs), dim3(64), 0, stream, cmds, cmd_off, scale, n_glyphs, cmd_open, error_flag,
	                   (const uint8_t *)nullptr, (const float *)nullptr, (const uint32_t *)nullptr, (OutlineCmd *)nullptr);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_outline_context_packed(const uint8_t *kinds, const float *coords, const uint32_t *dat_off, const uint32_t *cmd_off,
                                            const double *scale, uint32_t n_glyphs, OutlineCmd *cmds_out, uint8_t *cmd_open,
                                            uint32_t *error_flag, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	hipLaunchKernelGGL(outline_context<true>, dim3(n_glyphs), dim3(64), 0, stream, (const OutlineCmd *)nullptr, cmd_off, scale, n_glyphs,
	                   cmd_open, error_flag, kinds, coords, dat_off, cmds_out);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_outline_count(const OutlineCmd *cmds, const uint8_t *cmd_open, uint32_t n_cmds, const uint32_t *cmd_off,
                                   uint32_t n_glyphs, const double *scale, const double *shift_x, uint32_t *counts, void *cmd_box,
                                   unsigned long long *cmd_mask, uint32_t *error_flag, hipStream_t stream)
{
	if (n_cmds == 0)
		return 0;
	hipLaunchKernelGGL(outline_count, dim3((n_cmds + kFlattenThreads - 1) / kFlattenThreads), dim3(kFlattenThreads), 0, stream, cmds,
	                   cmd_open, n_cmds, cmd_off, n_glyphs, scale, shift_x, counts, (double4 *)cmd_box, cmd_mask, error_flag);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_outline_rings(const OutlineCmd *cmds, const uint32_t *cmd_off, const uint8_t *cmd_open, const double *scale,
                                   const double *shift_x, uint32_t n_glyphs, const uint32_t *counts, uint32_t *pt_local,
                                   const void *cmd_box, RingRec *rings, uint32_t *cmd_ring, OutlineRect *rects,
                                   uint32_t *error_flag, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	hipLaunchKernelGGL(outline_rings, dim3(n_glyphs), dim3(64), 0, stream, cmds, cmd_off, cmd_open, scale, shift_x, n_glyphs, counts, pt_local,
	                   (const double4 *)cmd_box, rings, cmd_ring, rects, error_flag);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_outline_emit_segments(const OutlineCmd *cmds, uint32_t n_cmds, const uint8_t *cmd_open, const double *scale,
                                           const double *shift_x,
                                           const uint32_t *pt_local, const RingRec *rings, const uint32_t *cmd_ring,
                                           const GlyphDesc *descs, const PlanHeader *hdr, unsigned long long seg_cap, double *seg,
                                           const unsigned long long *cmd_mask, uint32_t n_box_glyphs, const uint32_t *cmd_off,
                                           const void *cmd_box, void *boxes, hipStream_t stream)
{
	if (n_cmds == 0)
		return 0;
	hipLaunchKernelGGL(outline_emit_segments, dim3(n_box_glyphs + (n_cmds + kFlattenThreads - 1) / kFlattenThreads), dim3(kFlattenThreads), 0,
	                   stream, cmds, n_cmds, cmd_open, scale, shift_x, pt_local, rings, cmd_ring, descs, hdr, seg_cap, (double2 *)seg, cmd_mask,
	                   n_box_glyphs, cmd_off, (const double4 *)cmd_box, (float4 *)boxes);
	return (int)hipGetLastError();
}
