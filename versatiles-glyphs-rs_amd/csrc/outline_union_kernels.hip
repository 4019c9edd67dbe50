// outline_union_kernels.hip — the union pass (outline_union_kernels.h): a glyph's segments -> the boundary of
// { p : wn(p) != 0 }, rule U of DESIGN.md §7.  All arithmetic is f64 and this unit is built with -ffp-contract=off: every
// product, difference and quotient below is one IEEE operation, in the order tests/union_outline_kit.py restates, so the
// pieces can be compared bit for bit.  The count and the emit pass are one text (outline_union_pass.inc); the pieces are
// stored with plain vector stores.
#include "outline_union_kernels.h"

namespace vgsdf {
namespace {

constexpr uint32_t kUnionLanes = 256;

struct Seg {
	double sx, sy, ex, ey;
};
__device__ __forceinline__ bool zero_length(const Seg &s) { return s.sx == s.ex && s.sy == s.ey; } // takes no part

// The pair (k, p) is computed from its member of lower index i whichever of the two asks (U2): r = s_j - s_i, den = d_i x d_j,
// t along i and u along j.  -> den and cu = r x d_i (both zero: the two are coincident); ct = r x d_j
struct PairOf {
	Seg I, J;
	double dix, diy, djx, djy, den, cu, ct;
	__device__ __forceinline__ PairOf(const Seg &K, uint32_t k, const Seg &P, uint32_t p)
	{
		const bool lo = p < k;
		I = lo ? P : K, J = lo ? K : P;
		dix = I.ex - I.sx, diy = I.ey - I.sy, djx = J.ex - J.sx, djy = J.ey - J.sy;
		const double rx = J.sx - I.sx, ry = J.sy - I.sy;
		den = dix * djy - diy * djx;
		ct = rx * djy - ry * djx;
		cu = rx * diy - ry * dix;
	}
};

// Partner p's cuts of segment k: where the two cross, the point both use (an end point as it stands where a parameter is
// exactly 0 or 1, else s_i + t d_i); of a coincident partner its two end points, by k's dominant axis.  Takes a cut whose
// parameter on k lies in (cur_t, best_t).
__device__ __forceinline__ void next_cut(const Seg &K, uint32_t k, double dkx, double dky, const Seg &P, uint32_t p, double cur_t,
                                         double &best_t, double &bx, double &by)
{
	const PairOf q(K, k, P, p);
	if (q.den != 0.0) {
		const double t = q.ct / q.den, u = q.cu / q.den;
		if (t >= 0.0 && t <= 1.0 && u >= 0.0 && u <= 1.0) {
			const double tk = p < k ? u : t;
			if (tk > cur_t && tk < best_t) {
				double x = q.I.sx + t * q.dix, y = q.I.sy + t * q.diy;
				if (t == 0.0)
					x = q.I.sx, y = q.I.sy;
				else if (t == 1.0)
					x = q.I.ex, y = q.I.ey;
				else if (u == 0.0)
					x = q.J.sx, y = q.J.sy;
				else if (u == 1.0)
					x = q.J.ex, y = q.J.ey;
				best_t = tk, bx = x, by = y;
			}
		}
	} else if (q.cu == 0.0) {
		const bool by_x = fabs(dkx) >= fabs(dky);
		const double ts = by_x ? (P.sx - K.sx) / dkx : (P.sy - K.sy) / dky;
		if (ts > cur_t && ts < best_t)
			best_t = ts, bx = P.sx, by = P.sy;
		const double te = by_x ? (P.ex - K.sx) / dkx : (P.ey - K.sy) / dky;
		if (te > cur_t && te < best_t)
			best_t = te, bx = P.ex, by = P.ey;
	}
}

// Partner p's part in the classification of a piece of segment k at its midpoint (mx, my), in the frame of k's ray (steep:
// as it stands; else x and y exchanged): the reference's half-open crossing rule.  A coincident partner that straddles the
// midpoint belongs to k's group: it adds to the step and stays out of w.
__device__ __forceinline__ void classify(const Seg &K, uint32_t k, const Seg &P, uint32_t p, bool steep, double mx, double my, int sg,
                                         int &w, int &step, bool &lower_same)
{
	const double SX = steep ? P.sx : P.sy, SY = steep ? P.sy : P.sx, EX = steep ? P.ex : P.ey, EY = steep ? P.ey : P.ex;
	const int sign = (SY <= my && EY > my) ? 1 : ((SY > my && EY <= my) ? -1 : 0);
	if (sign == 0)
		return;
	const PairOf q(K, k, P, p);
	if (q.den == 0.0 && q.cu == 0.0) {
		step += sign;
		lower_same |= p < k && sign == sg;
	} else {
		const double t = (my - SY) / (EY - SY);
		const double x = SX + t * (EX - SX);
		if (x > mx)
			w += sign;
	}
}

template <bool EMIT>
__global__ __launch_bounds__(kUnionLanes) void outline_union_pass(const GlyphDesc *__restrict__ glyphs, const double *__restrict__ sx,
                                                                  const double *__restrict__ sy, const double *__restrict__ ex,
                                                                  const double *__restrict__ ey, uint32_t seg_stride, uint32_t *piece_count,
                                                                  uint8_t *state, uint32_t *seg_first, const uint32_t *__restrict__ piece_off,
                                                                  double *out_sx, double *out_sy, double *out_ex, double *out_ey,
                                                                  uint32_t out_stride)
{
#include "outline_union_pass.inc"
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_outline_union_count(const vgsdf::GlyphDesc *glyphs, uint32_t n_glyphs, const double *sx, const double *sy, const double *ex,
                              const double *ey, uint32_t seg_stride, uint32_t *piece_count, uint8_t *state, uint32_t *seg_first,
                              hipStream_t stream)
{
	if (!n_glyphs)
		return 0;
	hipLaunchKernelGGL(vgsdf::outline_union_pass<false>, dim3(n_glyphs), dim3(vgsdf::kUnionLanes), 0, stream, glyphs, sx, sy, ex, ey,
	                   seg_stride, piece_count, state, seg_first, (const uint32_t *)nullptr, (double *)nullptr, (double *)nullptr,
	                   (double *)nullptr, (double *)nullptr, 1u);
	return (int)hipGetLastError();
}

int vgsdf_outline_union_emit(const vgsdf::GlyphDesc *glyphs, uint32_t n_glyphs, const double *sx, const double *sy, const double *ex,
                             const double *ey, uint32_t seg_stride, const uint8_t *state, const uint32_t *seg_first,
                             const uint32_t *piece_off, double *out_sx, double *out_sy, double *out_ex, double *out_ey, uint32_t out_stride,
                             hipStream_t stream)
{
	if (!n_glyphs)
		return 0;
	hipLaunchKernelGGL(vgsdf::outline_union_pass<true>, dim3(n_glyphs), dim3(vgsdf::kUnionLanes), 0, stream, glyphs, sx, sy, ex, ey,
	                   seg_stride, (uint32_t *)nullptr, const_cast<uint8_t *>(state), const_cast<uint32_t *>(seg_first), piece_off, out_sx,
	                   out_sy, out_ex, out_ey, out_stride);
	return (int)hipGetLastError();
}

} // extern "C"
