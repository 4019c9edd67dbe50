// ---------------------------------------------------------------------------------------
// sdf_span_kernel.inc — the default raster kernel (public variant 0): bounded groups over SPANS.
// Included by sdf_kernels.hip once as `sdf_tiles_span` (the product) and, in development builds only, a second
// time as `sdf_tiles_span_stamped` with VG_STAMP / VG_COUNT switched on (s_memtime stamps per phase and a few
// counters, summed into g_span_dbg): the product instance carries no diagnostic argument, branch or register.
//
// Unit of work of a workgroup: up to SPAN_TILES = 4 consecutive 256-pixel tiles of ONE glyph.  A chunk of 256
// segments is staged (f64 loads, f32 records, row crossings, group bounds) ONCE and then swept by the span's tiles
// one after the other, so a glyph of <= 1024 pixels (99.7 % of Noto Sans) reads its segments from HBM/L2 once and
// pays the staging arithmetic once.  Per-pixel state between chunks (upper bound of the squared distance, the two
// candidate bytes) lives in LDS.
//   tiles[i] = SpanRec (sdf_kernels.h): the glyph's descriptor, its index, and first pixel | T: T in 1..4 tiles, chosen by
//   the list builder so that the rows the span touches fit the winding histogram.
// Because quantisation is monotone in the distance, the minimum over chunks can be taken on the BYTES: outside the
// nearest segment gives the largest byte, inside the smallest; both are kept until the winding number (complete
// only after the last chunk) picks one.  DESIGN.md §4.1 holds the exactness argument.
// ---------------------------------------------------------------------------------------
#ifndef VG_POOL_MAX
#define VG_POOL_MAX 2  // undecided lanes of a wave up to which their exact evaluation is pooled over the wave (0: never)
#endif
#ifndef VG_SPAN_KERNEL
#define VG_SPAN_KERNEL sdf_tiles_span
#endif
#ifndef VG_STAMP
#define VG_STAMP(region)
#endif
#ifndef VG_COUNT
#define VG_COUNT(stmt)
#endif
// ---- The numerical margins the exactness argument rests on (DESIGN.md §4.1), by name.  The defaults ARE the product:
// the product instance compiles to the same instructions as with the literals in place (profiles/raster_margins_isa_ab.txt).
// Only the margin instances of `make margins` (sdf_margin_kernels.hip) override one, each an arithmetic change only (a
// constant, or the outcome of a float comparison), to measure whether the suite notices a margin that is wrong.
// (h(F)'s own constants: VG_HERR_* / VG_E64_C in sdf_span_support.h.) ----
#ifndef VG_M_BOX_PADK
#define VG_M_BOX_PADK(mag) (0.02f + 2.0e-6f * (mag)) // chunk-box skip: f32 roundings of box and pixel centres
#endif
#ifndef VG_M_BOX_SAT
#define VG_M_BOX_SAT 6.2f // chunk-box skip: SAT
#endif
#ifndef VG_M_BOX_R
#define VG_M_BOX_R(r) (r) // chunk-box skip: the reach R = SAT + padk
#endif
#ifndef VG_M_BOX_BAND
#define VG_M_BOX_BAND(dy) ((dy) > 0.0f) // chunk-box skip: the box lies strictly outside the span's band of sample rows
#endif
#ifndef VG_M_INFL
#define VG_M_INFL (1.0f + 1.0f / 512.0f) // phase 1: inflation of U and r_g
#endif
#ifndef VG_M_GRP_SLACK
#define VG_M_GRP_SLACK 1.004f // phase 1: (U + r_g) against the bf16-packed D_g^2
#endif
#ifndef VG_M_PAD
#define VG_M_PAD(Mc) (0.01f + 1.0e-5f * (Mc)) // phase 1: absolute pad of U and r_g
#endif
#ifndef VG_M_RG
#define VG_M_RG(r) (r) // phase 1: the group radius in the candidate rule D_g <= U + r_g
#endif
#ifndef VG_M_SAT
#define VG_M_SAT 6.2f // phase 1: beyond it the byte is saturated (5.97 px outside / 2.02 px inside)
#endif
#ifndef VG_M_SANE
#define VG_M_SANE(Mc) ((Mc) < 1.0e6f) // the f32 filter is used at all
#endif
#ifndef VG_M_BOUNDED
#define VG_M_BOUNDED(Mc) ((Mc) < 4096.0f) // the group bounds are used
#endif
#ifndef VG_M_MABS0
#define VG_M_MABS0(m) (m) // largest absolute coordinate of the bitmap (e64)
#endif
#ifndef VG_M_E64
#define VG_M_E64(e) (e) // the reference's own f64 error against the real distance
#endif
#ifndef VG_M_E
#define VG_M_E(e) (e) // h(F) + e64 as used in decide, in the carried bound and in Tk
#endif
#ifndef VG_M_CARRY
#define VG_M_CARRY (1.0f + 1.0f / 1048576.0f) // carried bound ub2 = (f1 + e) (1 + 2^-20)
#endif
#ifndef VG_M_DL
#define VG_M_DL(dl) (dl) // decide: distance of s from the next integer that the interval needs
#endif
#ifndef VG_M_DL_C
#define VG_M_DL_C 17.0f // decide: dl = 17 e / sqrt(f1) + 3e-4
#endif
#ifndef VG_M_DL_ABS
#define VG_M_DL_ABS 3.0e-4f
#endif
#ifndef VG_M_E8
#define VG_M_E8(e, f1) (8.0f * (e) <= (f1)) // decide: the sqrt bound behind dl holds
#endif
#ifndef VG_M_FAR
#define VG_M_FAR 35.9f // decide: both bytes saturated beyond it
#endif
#ifndef VG_M_TK_PUSH
#define VG_M_TK_PUSH(tk) ((tk) * 1.001f + 1e-30f) // fallback threshold: pushed up behind the iteration
#endif
#ifndef VG_M_TK
#define VG_M_TK(tk, f1) (tk) // fallback threshold as used by the exact evaluation
#endif
#ifndef VG_M_ROW_E
#define VG_M_ROW_E(e) (e) // stage: distance of an f32 end point from a row centre below which the f64 brackets decide
#endif

__global__ __launch_bounds__(TPB, 4) void VG_SPAN_KERNEL(const SpanRec *__restrict__ tiles, uint32_t n_tiles,
                                                          const double *__restrict__ seg_sx,
                                                          const double *__restrict__ seg_sy,
                                                          const double *__restrict__ seg_ex,
                                                          const double *__restrict__ seg_ey, uint32_t seg_stride,
                                                          uint8_t *__restrict__ out, const float4 *__restrict__ boxes,
                                                          const PlanHeader *__restrict__ plan)
{
#ifdef VG_SPAN_STAMPED
	unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, st_last = 0;
#endif
#if defined(VG_SPAN_STAMPED) || defined(VG_SPAN_COUNTED)
	unsigned long long cn_pairs = 0, cn_rounds = 0, cn_tc = 0, cn_fb = 0, cn_fbl = 0;
	unsigned long long cn_over = 0, cn_fb_pool = 0, cn_fb_lane = 0; // phase-2 pool overflows; waves by exact-evaluation branch
	unsigned long long cn_half = 0, cn_leave = 0;                   // half rounds taken; sweeps that left behind phase 1 without a pair
	unsigned long long cn_row_fb = 0;                               // stage: waves of a chunk whose f64 brackets ran
#endif
	VG_STAMP(-1);
	// A workgroup's way to its first segment is two round trips of scalar loads and one of vector loads: the kernel
	// arguments; the work-list entry (which carries the glyph's descriptor) together with the plan's verdict; the segments
	// of chunk 0 behind the first barrier.  Every argument is named here, so that none is fetched later behind a wait of
	// its own.
	asm volatile("" ::"s"(seg_sx), "s"(seg_sy), "s"(seg_ex), "s"(seg_ey), "s"(seg_stride), "s"(out), "s"(boxes));
	const uint32_t tile = xcd_remap(blockIdx.x, n_tiles);
	// Behind the device front-end the launch is enqueued before the host has seen the plan: the grid is a guess
	// (>= the work list, or the plan says "not ok": some capacity was too small and the host launches again).  The entry
	// is read beside the verdict, not behind it: the grid never exceeds the list's capacity, and nothing of an entry is
	// used before the check below.  The empty statement is where both loads must have arrived: one wait for the two.
	const plan_ptr verdict = plan != nullptr ? (plan_ptr)plan : (plan_ptr)&k_plan_absent;
	uint32_t plan_ok = verdict->ok, plan_n_main = verdict->n_main;
	SpanRec g = tiles[tile];
	asm volatile(""
	             : "+s"(plan_ok), "+s"(plan_n_main), "+s"(g.seg_off), "+s"(g.n_seg), "+s"(g.x0), "+s"(g.y0), "+s"(g.w), "+s"(g.h), "+s"(g.out_off),
	               "+s"(g.first), "+s"(g.glyph));
	if (!plan_ok || blockIdx.x >= plan_n_main)
		return;
	constexpr uint32_t GRP = 8, NGRP = FCHUNK / GRP; // 32 groups per chunk: one mask bit each
	static_assert(NGRP == 32 && TPB == FCHUNK, "one candidate bit per group, one staging thread per record");
	// (arrays of one kind are rows of ONE array: the compiler keeps a thread's address into each LDS array in a VGPR for
	// the whole kernel, and the kernel sits at the 128-VGPR limit of 4 waves per SIMD)
	__shared__ __attribute__((aligned(16))) float s_rec[5][FCHUNK]; // f32 records: v - origin (x, y), d = w - v (x, y), 1 / |d|^2
	__shared__ double e_pt[4][FCHUNK];                              // exact end points: v.x, v.y, w.x, w.y
	float *const s_vx = s_rec[0], *const s_vy = s_rec[1], *const s_dx = s_rec[2], *const s_dy = s_rec[3], *const s_inv = s_rec[4];
	double *const e_vx = e_pt[0], *const e_vy = e_pt[1], *const e_wx = e_pt[2], *const e_wy = e_pt[3];
	__shared__ int s_delta[DELTA_CAP];
	__shared__ uint32_t s_mbits[2]; // coordinate bound of the chunk being staged (slot = parity of processed chunks)
	__shared__ __attribute__((aligned(16))) float s_g[3][NGRP]; // per group: anchor x, anchor y, radius (one array: one address register)
	// per wave: the groups that survive the wave-level cull, compacted (4 pad entries behind the last one)
	__shared__ float st_ub2[SPAN_TILES * TPB];    // per pixel: upper bound of the squared distance so far
	__shared__ uint16_t st_byte[SPAN_TILES * TPB]; // per pixel: byte if inside (low), byte if outside (high)
	__shared__ uint32_t st_pix[SPAN_TILES * TPB];  // per pixel: its coordinates (pix_pack, sdf_span_support.h), divided out once
	constexpr uint32_t QCAP = 256;                 // pooled (pixel, group) pairs per wave and sweep; beyond: per-lane walk
	// a pooled pair is its two LDS byte offsets: (4 lane) << 16 (the lane's ds_bpermute address and its q_min slot) | 32 group
	// (the group's first record in a row of s_rec).  The stage's row crossings pool (lane << 10) | row in the same entries.
	__shared__ uint32_t q_pair[TPB / 64][QCAP];
	__shared__ uint32_t q_min[TPB / 64][64];       // per pixel of the wave: smallest filter value (bits)

	const uint32_t tid = threadIdx.x, lane = threadIdx.x & 63;
	const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // wave-uniform: addresses of the per-wave LDS rows stay scalar
	// The 64-pixel quarters of a tile go to the waves rotated by `rot` (0..3, a hash of the workgroup's index): wave wv takes
	// the pixels from pw of every tile, in the sweep and in the final stores.  Only a glyph's last tile is partial and its
	// empty quarters are the last ones, so unrotated the waves with the high numbers sweep less than wave 0 in every
	// workgroup (tools/model_wave_shares.py).  Whatever is indexed by tid (the stage's records, st_ub2, st_byte) stays put.
	const uint32_t rot = wave_rot(blockIdx.x);
	const uint32_t pw = ((wv + rot) & 3u) * 64u;
	const uint32_t npix = g.w * g.h;
	const uint32_t p0 = g.first & ~255u, T = min(max(g.first & 255u, 1u), SPAN_TILES);
	const uint32_t p_end = min(p0 + T * (uint32_t)TPB, npix); // pixels [p0, p_end) of the glyph's bitmap

	const uint32_t r_first = p0 / g.w, r_last = (p_end - 1) / g.w;
	const int y_hi = (int)(g.h - 1 - r_first), y_lo = (int)(g.h - 1 - r_last);
	// one histogram row = w + 1 cells (the last one collects "no column left of the pixel row's end"), padded to an odd
	// stride so that the per-row scans after the chunk loop (one thread per row) spread over the LDS banks
	const uint32_t stride = (g.w + 1) | 1u;
	const uint32_t n_delta = (r_last - r_first + 1) * stride; // <= DELTA_CAP (host-checked)
	for (uint32_t i = tid; i < n_delta; i += TPB)
		s_delta[i] = 0;
	const float wh = (float)max(g.w, g.h);
	// Origin of every f32 quantity of the filter (records, anchors, pixel centres): the middle of the bitmap,
	// an integer point.  The filter's error bound h(F) scales with M = the largest |coordinate| relative to
	// that origin, so the middle halves it against the corner (x0, y0) (and with it the share of pixels whose
	// byte needs the exact f64 evaluation).  Pixel centres stay exact in f32 (half-integers).
	const int hw = (int)(g.w >> 1), hh = (int)(g.h >> 1);
	// The pixel of thread tid in tile k is p0 + k TPB + pw + lane for the whole kernel: its column and row are divided
	// out here, once, and every sweep (one per chunk) and the final stores read them from st_pix.  A padding lane of
	// the last tile gets the bitmap's last pixel (it takes part in the wave's shuffles; its candidate mask is cleared
	// in the sweep and it stores nothing).  Each thread reads only what it wrote itself: no barrier.
	for (uint32_t k = 0; k < T; k++) {
		st_ub2[k * TPB + tid] = __builtin_inff();
		st_byte[k * TPB + tid] = 0x00FFu; // neutral: 255 for the min (inside), 0 for the max (outside)
		const uint32_t oc = min(p0 + k * TPB + pw + lane, npix - 1);
		const uint32_t row = oc / g.w; // r_first <= row <= r_last
		st_pix[k * TPB + tid] = pix_pack((float)((int)(oc - row * g.w) - hw) + 0.5f, row - r_first);
	}
	// the span's first row against the origin, as one opaque scalar (or the compiler re-derives it from h, r_first and hh per lane)
	int y_mid = y_hi - hh;
	asm volatile("" : "+s"(y_mid));
	const float mpix = 0.5f * wh + 1.0f; // >= |pixel centre - origin| in both axes
	uint32_t par = 0;
	if (tid == 0)
		s_mbits[0] = __float_as_uint(mpix);
	const float mabs0 = VG_M_MABS0(fmaxf(fmaxf(fabsf((float)g.x0), fabsf((float)g.y0)),
	                                     fmaxf(fabsf((float)g.x0 + (float)g.w), fabsf((float)g.y0 + (float)g.h))));

	// the box test pays for glyphs with several chunks; with one or two there is nothing to gain
	const bool use_boxes = boxes != nullptr && g.n_seg > 2 * FCHUNK;
	for (uint32_t c0 = 0; c0 < g.n_seg; c0 += FCHUNK) {
		const uint32_t cnt = min((uint32_t)FCHUNK, g.n_seg - c0);
		VG_STAMP(0); // prologue / loop overhead
		__syncthreads(); // previous chunk fully consumed (and s_delta / state initialised on the first trip)
		VG_STAMP(1); // wait at the chunk-top barrier
		if (use_boxes) {
			// ---- chunk box test (workgroup-uniform).  Skip the chunk if its box lies strictly outside the
			// span's band of sample rows (so none of its segments crosses one of them: no winding
			// contribution) AND farther than SAT from every pixel of the span: a segment beyond SAT is either
			// not the minimum, or the byte is saturated whatever the minimum is.  f32 roundings (box, pixel
			// centres) are covered by padk.  (Tightening R with the pixels' running upper bounds was
			// measured: the bookkeeping costs more than the extra skips on real fonts.) ----
			const float4 bb = boxes[chunk_box_index(g.seg_off, g.glyph, c0 / FCHUNK)];
			const float mag = fmaxf(fmaxf(fabsf(bb.x), fabsf(bb.y)), fmaxf(fmaxf(fabsf(bb.z), fabsf(bb.w)), wh));
			const float padk = VG_M_BOX_PADK(mag);
			const float ry0 = (float)y_lo + 0.5f, ry1 = (float)y_hi + 0.5f; // sample rows of the span, relative to y0
			const float dy = fmaxf(bb.y - ry1, ry0 - bb.w) - padk;
			float dx = fmaxf(bb.x - ((float)g.w - 0.5f), 0.5f - bb.z) - padk;
			dx = dx > 0.0f ? dx : 0.0f;
			const float R = VG_M_BOX_R(VG_M_BOX_SAT + padk); // SAT
			if (VG_M_BOX_BAND(dy) && __builtin_fmaf(dy, dy, dx * dx) > R * R)
				continue; // NaN anywhere -> comparison false -> the chunk is processed
		}
		// ---- stage (thread i <-> record i): exact endpoints, f32 record, coordinate bound, group bounds,
		// row crossings.  Everything a thread needs from other threads here comes from lanes of its own wave
		// (a group of 8 records, the crossings of the wave's 64 segments), so there is one workgroup barrier
		// behind the stage and none inside it. ----
		constexpr float INFL = VG_M_INFL;
		{
			// Workgroup-uniform f64 values of the stage (there is no scalar f64 unit: each would occupy a VGPR pair for the
			// whole kernel, and the kernel sits at the 128-VGPR limit of 4 waves per SIMD): formed here, behind a barrier
			// the compiler cannot hoist them across, from the integers they come from.
			int gx0 = g.x0, gy0 = g.y0;
			asm volatile("" : "+s"(gx0), "+s"(gy0));
			const double ox = (double)gx0 + (double)hw, oy = (double)gy0 + (double)hh;
			const uint32_t i = tid;
			float mf = 0.0f;
			float fvx = 1.0e18f, fvy = 1.0e18f, fdx = 0.0f, fdy = 0.0f, finv = 0.0f; // padding: a record that can never win (F = 2e36)
			uint32_t nrow = 0; // sample rows of the span this thread's segment crosses: yy in [ya, ya + nrow)
			int ya = 0;
			bool row_exact = false; // the f32 record does not fix the brackets: first_ge does, below
			if (i < cnt) {
				const size_t s = (size_t)(g.seg_off + c0 + i) * seg_stride; // stride 1: SoA arrays; 4: {sx, sy, ex, ey} records
				// (issued here, behind the chunk-top barrier.  Chunk 0's loads issued at the top of the kernel, under the rest of the
				// prologue, were built and measured: slower; a later chunk's above the barrier spill: profiles/span_startup_ab.txt)
				const double vx = seg_sx[s], vy = seg_sy[s], wx = seg_ex[s], wy = seg_ey[s];
				e_vx[i] = vx;
				e_vy[i] = vy;
				e_wx[i] = wx;
				e_wy[i] = wy;
				const double dx = wx - vx, dy = wy - vy;
				const double l2 = dx * dx + dy * dy;
				fvx = (float)(vx - ox);
				fvy = (float)(vy - oy);
				fdx = (float)dx;
				fdy = (float)dy;
				// 1 / |d|^2 to ~3 units of f32 roundoff (conversion + v_rcp_f32): the closest point of the f32 record
				// moves by <= 17 u M along the segment, inside the 28.6 u M the filter's error bound h(F) allows
				finv = (l2 > 1e-20 && l2 < 1e30) ? __builtin_amdgcn_rcpf((float)l2) : 0.0f;
				// coordinate bound from the f32 values (end point as v + d: <= 2.5 ulp(M) off), rounded up
				mf = fmaxf(fmaxf(fabsf(fvx), fabsf(fvy)), fmaxf(fabsf(fvx + fdx), fabsf(fvy + fdy))) * 1.00001f;
				mf = mf >= 0.0f ? mf : __builtin_inff(); // NaN -> inf ("no usable bound")
				// crossings, renderer_precise.rs:41-51: up (+1) s.y <= py < e.y; down (-1) e.y <= py < s.y.
				// Rows crossed: lo <= py < hi with py = yy + y0c exactly as the reference forms it.
				// The brackets from the f32 record first.  Row n lies at n - hh + 1/2 against the origin, so first_ge(y) =
				// ceil(t) + hh with t = (y - oy) - 1/2, clamped; tv and tw are t of the two end points to within E_row
				// (DESIGN.md §4.1), and ceil is monotone, so the smaller one is lo's whichever way the segment runs.  Farther
				// than E_row from every integer, both are the exact brackets, and the clamps to the span's rows do what
				// the band test does.  mf = inf (a NaN or an infinity in the record) or >= 10^6 leaves the lane to first_ge.
				const float tv = fvy - 0.5f, tw = (fvy + fdy) - 0.5f;
				const float e_row = VG_M_ROW_E(__builtin_fmaf(STAGE_ROW_C, fmaxf(mf, mpix), STAGE_ROW_ABS));
				const bool decided = __builtin_fminf(int_dist(tv), int_dist(tw)) > e_row && mf < STAGE_M_MAX;
				const int cv = (int)__builtin_ceilf(tv), cw = (int)__builtin_ceilf(tw);
				const int c_lo = y_lo - hh, c_hi = y_hi + 1 - hh;
				const int ca = min(max(min(cv, cw), c_lo), c_hi), cb = min(max(max(cv, cw), c_lo), c_hi);
				ya = ca + hh;
				nrow = decided ? (uint32_t)(cb - ca) : 0u;
				row_exact = vy != wy && !decided; // (a level segment crosses no row wherever it lies: tv == tw)
			}
			const bool row_fb = __builtin_amdgcn_ballot_w64(row_exact) != 0; // wave-uniform: the f64 brackets are skipped, not masked
			VG_COUNT(cn_row_fb += row_fb);
			if (row_fb && row_exact) {
				// Most segments of a real font are a fraction of a pixel tall and most lie outside the span's band of rows:
				// two exact compares reject those before the integer brackets are computed.
				const double vy = e_vy[i], wy = e_wy[i]; // (this thread's own stores)
				const double y0c = (double)gy0 + 0.5;    // renderer_precise.rs:28
				const double band_lo = (double)y_lo + y0c, band_hi = (double)y_hi + y0c; // lowest / highest sample row of the span
				const bool up = vy < wy;
				const double lo = up ? vy : wy, hi = up ? wy : vy;
				if (hi > band_lo && lo <= band_hi) {
					ya = first_ge(lo, y0c, y_lo, y_hi + 1);
					const int yb = first_ge(hi, y0c, y_lo, y_hi + 1); // first row with py >= hi
					nrow = yb > ya ? (uint32_t)(yb - ya) : 0u;
				}
			}
			s_vx[i] = fvx;
			s_vy[i] = fvy;
			s_dx[i] = fdx;
			s_dy[i] = fdy;
			s_inv[i] = finv;
			// coordinate bound: wave maximum first, one LDS atomic per wave (non-negative floats order like uints)
			// (the maximum arrives as a scalar: lane 0's atomic then takes a wave-uniform value, nothing for the compiler to reduce)
			const uint32_t mb = wave_max_u32(__float_as_uint(mf));
			if (lane == 0)
				atomicMax(&s_mbits[par], mb);

			// ---- group bounds (8 consecutive records = 8 lanes): anchor = start vertex of the middle member, radius
			// over all end points.  The pad that depends on the workgroup's coordinate bound is added in phase 1. ----
			{
				const uint32_t gb = tid & ~(GRP - 1);
				const uint32_t ai = min(gb + GRP / 2, cnt - 1); // (a lane of this group whenever the group holds a record)
				const float ax = __shfl(fvx, (int)(ai & 63u)), ay = __shfl(fvy, (int)(ai & 63u));
				float r2 = 0.0f;
				if (i < cnt) {
					const float wx = fvx + fdx, wy = fvy + fdy;
					const float ex = fvx - ax, ey = fvy - ay, fx = wx - ax, fy = wy - ay;
					const float dv = __builtin_fmaf(ey, ey, ex * ex), dw = __builtin_fmaf(fy, fy, fx * fx);
					r2 = dv > dw ? dv : dw;
				}
				// maximum over the group's 8 lanes on the bits (r2 >= +0: unsigned order is float order; a NaN, which only
				// coordinates beyond the f32 range produce, stays a NaN, and Mc = inf then switches the group bounds off)
				r2 = __uint_as_float(oct_max_u32(__float_as_uint(r2)));
				if ((tid & (GRP - 1)) == 0) {
					const bool empty = gb >= cnt;
					s_g[0][tid / GRP] = empty ? 1.0e18f : ax;
					s_g[1][tid / GRP] = empty ? 1.0e18f : ay;
					// (raw v_sqrt_f32: within 1 ulp of the rounded root, 0 for a denormal r2 < 1.2e-38; INFL and the pad of phase 1 cover both)
					s_g[2][tid / GRP] = empty ? 0.0f : __builtin_amdgcn_sqrtf(r2) * (INFL * INFL * VG_M_GRP_SLACK); // 1.004: see phase 1
				}
			}

			// ---- row crossings of the wave's 64 segments, one (segment, row) pair per lane and round: a vertical stem
			// crosses 20 rows, its neighbours none, and a per-thread loop would keep the whole workgroup waiting
			// at the barrier for the one long segment (2.6 trips per wave on average, up to 24, against 7.5
			// crossings per wave in total). ----
			{
				const uint32_t incl = wave_scan_add(nrow); // inclusive prefix sum over the wave
				const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
				auto cross = [&](double vx, double vy, double dx, double dy, bool up, int yy) {
					const double x0c = (double)gx0 + 0.5, y0c = (double)gy0 + 0.5; // renderer_precise.rs:27-28
					const double pyy = (double)yy + y0c;
					const double tc = (pyy - vy) / dy;
					const double xc = vx + tc * dx;               // :45-46 / :48-49
					const int k = first_ge(xc, x0c, 0, (int)g.w); // first column with xc <= px (:63)
					if (k < (int)g.w)
						atomicAdd(&s_delta[(uint32_t)(y_hi - yy) * stride + (uint32_t)k], up ? -1 : 1); // wn -= sign
				};
				if (total != 0 && total <= QCAP) {
					// (lane, row) pairs of the wave, pooled in LDS (rows of a span: < 1024, host-checked through DELTA_CAP)
					// (not unrolled: a wave's longest segment crosses two or three rows on a font, and the unrolled loop's
					// entry checks cost more than its trips)
					uint32_t off = incl - nrow;
#pragma unroll 1
					for (uint32_t r = 0; r < nrow; r++)
						q_pair[wv][off++] = (lane << 10) | (uint32_t)(y_hi - (ya + (int)r));
					__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
					__builtin_amdgcn_wave_barrier();
					for (uint32_t base = 0; base < total; base += 64) {
						const uint32_t idx = base + lane;
						if (idx < total) {
							const uint32_t e = q_pair[wv][idx];
							const uint32_t si = (tid & ~63u) + (e >> 10); // the segment's record (staged by this wave)
							const double vx = e_vx[si], vy = e_vy[si], wx = e_wx[si], wy = e_wy[si];
							cross(vx, vy, wx - vx, wy - vy, vy < wy, y_hi - (int)(e & 1023u));
						}
					}
					__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
					__builtin_amdgcn_wave_barrier();
				} else if (total != 0) { // more pairs than the pool holds (tall glyphs): every thread walks its own rows
					if (nrow != 0) {
						const double vx = e_vx[i], vy = e_vy[i], wx = e_wx[i], wy = e_wy[i];
						for (uint32_t r = 0; r < nrow; r++)
							cross(vx, vy, wx - vx, wy - vy, vy < wy, ya + (int)r);
					}
				}
			}
		}
		VG_STAMP(2); // stage: loads, records, crossings, coordinate bound, group bounds
		__syncthreads();
		VG_STAMP(3); // wait at the post-stage barrier
		const float Mc = __uint_as_float(s_mbits[par]);
		par ^= 1u;
		if (tid == 0)
			s_mbits[par] = __float_as_uint(mpix); // the next processed chunk's accumulator (nobody touches it before the next chunk-top barrier)
		const bool sane = VG_M_SANE(Mc);   // else: no usable f32 bound -> every segment is evaluated exactly
		const bool bounded = VG_M_BOUNDED(Mc); // group bounds have a useful margin
		const float pad = VG_M_PAD(Mc);
		const uint32_t n_groups = (cnt + GRP - 1) / GRP;

		const float4 *q_vx = reinterpret_cast<const float4 *>(s_vx), *q_vy = reinterpret_cast<const float4 *>(s_vy);
		const float4 *q_dx = reinterpret_cast<const float4 *>(s_dx), *q_dy = reinterpret_cast<const float4 *>(s_dy);
		const float4 *q_inv = reinterpret_cast<const float4 *>(s_inv);
		const float M = Mc;
		const float e64 = VG_M_E64(VG_E64_C * M * (M + mabs0 + M)); // 2^-44 M (M + Mabs)
		// h(F) + e64 as one fused expression in the decide step: h(F) = 1.001 (64 u M sqrt(F) + 32 u F + 2^-34 M^2)
		const float herr_c1 = VG_HERR_SLACK * VG_HERR_C1 * M, herr_c3 = VG_HERR_SLACK * VG_HERR_C3 * M * M + e64;

		// ---- sweep: every tile of the span against the staged chunk ----
#pragma unroll 1
		for (uint32_t k = 0; k < T; k++) {
			// compiler barrier: keeps the (loop-invariant, wave-uniform) group-bound loads inside the loop
			// instead of parking 96 VGPRs of them across it
			asm volatile("" ::: "memory");
			const uint32_t o = p0 + k * TPB + pw + lane;
			// a wave whose 64 pixels all lie past the end of the bitmap (last tile of the glyph) has nothing to do
			if (p0 + k * TPB + pw >= npix)
				continue;
			// pixel centre relative to the origin, from the table: column x = pix_col(rpx, hw), row y = y_hi - roff above y0
			const uint32_t pe = st_pix[k * TPB + tid];
			const float rpx = pix_rpx(pe);
			const int roff = (int)pix_roff(pe);
			const float rpy = (float)(y_mid - roff) + 0.5f; // (the integer first: the same rounding as (float)(y - hh) at any h)
			float ub2 = st_ub2[k * TPB + tid];
			VG_STAMP(0);


			// ---- phase 1: candidate groups of this lane ----
			uint32_t cand = n_groups >= 32 ? 0xFFFFFFFFu : ((1u << n_groups) - 1u);
			if (bounded) {
				// D_g^2 of two groups per register, upper 16 bits of each float (truncation: the stored value
				// is <= the true one; the high half read as a float is < true * (1 + 2^-7)): keeps the kernel
				// inside the 128-VGPR budget of 4 waves per SIMD.  The test below inflates U + r_g by 1.004
				// (> sqrt(1 + 2^-7)), so every true candidate still passes.
				uint32_t D2p[NGRP / 2];
				uint32_t dmin = __float_as_uint(ub2);
				const float4 *gx4 = reinterpret_cast<const float4 *>(s_g[0]), *gy4 = reinterpret_cast<const float4 *>(s_g[1]);
				const float4 *gr4 = reinterpret_cast<const float4 *>(s_g[2]);
				auto near4 = [&](uint32_t b, const float4 ax, const float4 ay) { // D_g^2 of the four groups of block b
					const float axs[4] = {ax.x, ax.y, ax.z, ax.w}, ays[4] = {ay.x, ay.y, ay.z, ay.w};
					uint32_t d2[4];
#pragma unroll
					for (int j = 0; j < 4; j++) {
						const float ddx = rpx - axs[j], ddy = rpy - ays[j];
						d2[j] = __float_as_uint(__builtin_fmaf(ddy, ddy, ddx * ddx));
					}
					// d2 >= +0: unsigned order of the bits is float order; one v_min3_u32 per two groups
					asm("v_min3_u32 %0, %1, %2, %3" : "=v"(dmin) : "v"(dmin), "v"(d2[0]), "v"(d2[1]));
					asm("v_min3_u32 %0, %1, %2, %3" : "=v"(dmin) : "v"(dmin), "v"(d2[2]), "v"(d2[3]));
					D2p[b * 2] = __builtin_amdgcn_perm(d2[1], d2[0], 0x07060302u);     // hi16(d2[1]) : hi16(d2[0])
					D2p[b * 2 + 1] = __builtin_amdgcn_perm(d2[3], d2[2], 0x07060302u);
				};
				// Both shapes issue a block's two anchor loads ahead of the arithmetic of the block before it: a wave
				// waits for an LDS round trip it has nothing to put in front of, whatever the other three waves of
				// its SIMD do (profiles/sweep_latency_ab.txt).  A full chunk runs the eight blocks in a straight line,
				// as the second pass does.  A partial chunk leaves at the first block past n_groups (a block past
				// n_groups leaves its D2p unset: the second pass skips the same blocks); the load issued ahead for
				// that block reads what the stage wrote for its empty groups (1e18 / 0 in every processed chunk).
				if (n_groups == NGRP) {
#pragma unroll
					for (uint32_t b = 0; b < NGRP / 4; b++)
						near4(b, gx4[b], gy4[b]);
				} else {
					float4 ax = gx4[0], ay = gy4[0];
#pragma unroll
					for (uint32_t b = 0; b < NGRP / 4; b++) {
						if (b * 4 < n_groups) {
							if (b + 1 == NGRP / 4) { // (unrolled: no condition is left in the code)
								near4(b, ax, ay);
								break;
							}
							const float4 nx = gx4[b + 1], ny = gy4[b + 1];
							near4(b, ax, ay);
							// (pins the two loads to this block: left alone the compiler sinks them into the next block, their only
							// user, where they are waited for at once)
							asm volatile("" ::"v"(nx.x), "v"(nx.y), "v"(nx.z), "v"(nx.w), "v"(ny.x), "v"(ny.y), "v"(ny.z), "v"(ny.w));
							ax = nx;
							ay = ny;
						} else {
							break;
						}
					}
				}
				ub2 = __uint_as_float(dmin);
				float U = (__builtin_amdgcn_sqrtf(ub2) * INFL + pad) * INFL; // (raw v_sqrt_f32, as for the group radius: DESIGN.md §4.1)
				U = U < VG_M_SAT ? U : VG_M_SAT; // SAT: beyond it the byte is saturated whatever the minimum is
				const float Ui = (U + pad * INFL) * VG_M_GRP_SLACK; // s_gr is stored with the same factor; it lacks the pad of r_g
				// One bit per group, 3-4 VALU ops each: tt = (U + r_g) 1.004, diff = tt^2 - D_g^2 (sign bit set
				// <=> not a candidate), shifted in with v_alignbit from the chunk's highest block of four down to
				// group 0, so group i lands on bit i however many blocks the chunk holds.
				// A full chunk (every chunk of a glyph but its last) runs all eight blocks in a straight line: the
				// eight loads of the radii are issued ahead of the arithmetic and their latency is paid once.
				// A partial chunk skips the blocks past n_groups by the first pass's workgroup-uniform condition
				// (scalar branches: the switch enters at the chunk's block count and falls through; each block
				// waits for its own load, which costs more than the skipped blocks save once all eight are real:
				// profiles/sweep_diet2_ab.txt).  There the bits above the real blocks' are whatever rej held
				// before: cand, which starts as the mask of the chunk's real groups, ignores them, so rej needs no
				// initial value (a constant costs up to two v_mov at every entry of the switch; the empty statement
				// below hands the compiler "some register" instead, one copy per entry passed).  The empty groups
				// inside the last real block have their anchors at 1e18 (D_g^2 = 2e36, finite: the pass stays
				// NaN-free) and radius 0, and lie outside cand too.
				uint32_t rej;
				asm volatile("" : "=v"(rej));
				auto reject4 = [&](uint32_t b) {
					const float4 r = gr4[b];
					const float rs[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
					for (int j = 3; j >= 0; j--) {
						const uint32_t pk = D2p[b * 2 + j / 2];
						const float d2 = __uint_as_float((j & 1) ? pk : (pk << 16));
						const float tt = Ui + VG_M_RG(rs[j]);
						const float diff = __builtin_fmaf(tt, tt, -d2);
						rej = __builtin_amdgcn_alignbit(rej, __float_as_uint(diff), 31); // (rej << 1) | sign(diff)
					}
				};
				static_assert(NGRP / 4 == 8, "one case per block of four groups");
				if (n_groups == NGRP) {
#pragma unroll
					for (int b = NGRP / 4 - 1; b >= 0; b--)
						reject4((uint32_t)b);
				} else switch ((n_groups + 3) / 4) { // 1..8 (a processed chunk holds a record)
				default: reject4(7); [[fallthrough]];
				case 7: reject4(6); [[fallthrough]];
				case 6: reject4(5); [[fallthrough]];
				case 5: reject4(4); [[fallthrough]];
				case 4: reject4(3); [[fallthrough]];
				case 3: reject4(2); [[fallthrough]];
				case 2: reject4(1); [[fallthrough]];
				case 1: reject4(0);
				}
				cand &= ~rej;
			}

			VG_STAMP(6); // phase 1
			// ---- phase 2: smallest f32 filter value over the lane's candidate groups (F >= +0: unsigned
			// order of the bits is float order) ----
			uint32_t k1 = 0xFFFFFFFFu;
			auto rec4 = [](const float4 *row, uint32_t goff, uint32_t hq) { // records 4 hq .. 4 hq + 3 of the group at byte goff of `row`
				return *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(row) + goff + 16u * hq);
			};
			auto half_min = [&](uint32_t acc, uint32_t goff, uint32_t hq, float qx, float qy) { // min(acc, F of records 4 hq .. 4 hq + 3 of the group at byte goff)
				const float4 vx4 = rec4(q_vx, goff, hq), vy4 = rec4(q_vy, goff, hq), dx4 = rec4(q_dx, goff, hq), dy4 = rec4(q_dy, goff, hq),
				             iv4 = rec4(q_inv, goff, hq);
				const uint32_t f0 = __float_as_uint(sc_filter(qx, qy, vx4.x, vy4.x, dx4.x, dy4.x, iv4.x));
				const uint32_t f1 = __float_as_uint(sc_filter(qx, qy, vx4.y, vy4.y, dx4.y, dy4.y, iv4.y));
				const uint32_t f2 = __float_as_uint(sc_filter(qx, qy, vx4.z, vy4.z, dx4.z, dy4.z, iv4.z));
				const uint32_t f3 = __float_as_uint(sc_filter(qx, qy, vx4.w, vy4.w, dx4.w, dy4.w, iv4.w));
				uint32_t mn;
				asm("v_min3_u32 %0, %1, %2, %3" : "=v"(mn) : "v"(acc), "v"(f0), "v"(f1));
				asm("v_min3_u32 %0, %1, %2, %3" : "=v"(acc) : "v"(mn), "v"(f2), "v"(f3));
				return acc;
			};
			auto group_min = [&](uint32_t acc, uint32_t goff, float qx, float qy) { // min(acc, F of the 8 members of the group at byte goff = 32 g of a row)
				// two halves of 4 records: 20 + 4 live values instead of 40 + 8 (the kernel sits at the 128-VGPR
				// limit of 4 waves per SIMD; spills would go to scratch, i.e. to memory)
				acc = half_min(acc, goff, 0, qx, qy);
				__builtin_amdgcn_sched_barrier(0);
				return half_min(acc, goff, 1, qx, qy);
			};
			if (sane) {
				if (o >= npix)
					cand = 0; // padding lanes of the last tile own no pixel
				// The lanes of a wave hold very different numbers of candidate groups (mean 1.7 per chunk,
				// busiest lane 4-5).  Instead of every lane walking its own list while the others idle, the
				// wave pools its (pixel, group) pairs in LDS and deals them out evenly: 64 pairs per round,
				// results merged with ds_min_u32 on the owning pixel's slot.
				const uint32_t c = (uint32_t)__builtin_popcount(cand);
				const uint32_t incl = wave_scan_add(c); // inclusive prefix sum over the wave
				const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
				VG_COUNT(cn_pairs += total; cn_rounds += (total + 63) / 64; cn_tc += 1);
				// No lane of the wave holds a candidate (wave-uniform; 18 % of the sweeps of Noto Sans): k1 stays "none" in every
				// lane, nothing is undecided and the bytes keep what they hold (min with 255, max with 0).  Only the bound,
				// which phase 1 may have lowered, is kept.
				if (total == 0) {
					st_ub2[k * TPB + tid] = ub2;
					VG_COUNT(cn_leave += 1);
					continue;
				}
				if (total <= QCAP) {
					uint32_t *qp = &q_pair[wv][incl - c];
					q_min[wv][lane] = 0xFFFFFFFFu;
					uint32_t m = cand;
					while (m) {
						*qp = (lane << 18) | ((uint32_t)__builtin_ctz(m) << 5);
						__builtin_amdgcn_sched_barrier(0); // (the store first: the pointer is then bumped in place, no copy)
						qp++;
						m &= m - 1;
					}
					__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
					__builtin_amdgcn_wave_barrier();
					// A last round of 1 .. 32 entries (40 % of the pooled sweeps end in one) is a HALF round: lanes l and l + 32
					// take entry l and four of the group's eight records each (one step of group_min), and both merge onto the
					// pixel's slot.  The full rounds in front of it are all full; `tail` and `lim` are wave-uniform.
					const uint32_t tail = ((total - 1u) & 63u) + 1u;
					const uint32_t lim = tail <= 32u ? total - tail : total; // entries of the full rounds
					// The entry of the round after this one is read before this round's filters: a round then waits for the
					// pixel and the records only, not for its entry first (the first round's is read ahead of the loop; past
					// the last round the read takes the last pair again: q_pair holds QCAP entries).  The half round's entry
					// arrives the same way.  The loop runs on the NEXT round's base, the only index a round forms: its own is
					// that minus 64.
					uint32_t e = q_pair[wv][min(lane, total - 1)]; // (a lane past the end takes the last pair and drops its result)
					const uint32_t lim64 = lim + 64;              // (total <= QCAP)
					for (uint32_t next = 64; next < lim64; next += 64) {
						const uint32_t idx_next = next + lane;
						const uint32_t e_next = q_pair[wv][min(idx_next, total - 1)];
						const uint32_t src4 = e >> 16;
						const float qx = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)src4, (int)__float_as_uint(rpx)));
						const float qy = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)src4, (int)__float_as_uint(rpy)));
						const uint32_t mn = group_min(0xFFFFFFFFu, e & 0xFFFFu, qx, qy);
						if (idx_next < lim64) // this round's index < lim
							atomicMin(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(q_min[wv]) + src4), mn);
						e = e_next;
					}
					if (lim != total) {
						VG_COUNT(cn_half += 1);
						// e is the entry lim + lane: the upper half of the wave takes the lower half's (v_permlane32_swap: lanes
						// 32..63 of the first operand <-> lanes 0..31 of the second).  A group's padding records (F = 2e36) lose
						// against the other half's real ones on the slot as they do inside group_min.
						const uint32_t eh = __builtin_amdgcn_permlane32_swap(e, e, false, false)[0];
						const uint32_t src4 = eh >> 16;
						const float qx = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)src4, (int)__float_as_uint(rpx)));
						const float qy = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)src4, (int)__float_as_uint(rpy)));
						const uint32_t mn = half_min(0xFFFFFFFFu, eh & 0xFFFFu, lane >> 5, qx, qy);
						if ((lane & 31u) < tail)
							atomicMin(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(q_min[wv]) + src4), mn);
					}
					__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
					__builtin_amdgcn_wave_barrier();
					k1 = q_min[wv][lane];
				} else {
					// (pooling such a sweep in passes over windows of QCAP pairs was built and measured: slower than this walk,
					// profiles/pair_rounds_ab.txt)
					VG_COUNT(cn_over += 1);
					uint32_t m = cand;
					while (m) {
						const uint32_t gq = (uint32_t)__builtin_ctz(m);
						m &= m - 1;
						k1 = group_min(k1, gq * 32u, rpx, rpy);
					}
				}
			}

			// ---- decide.  The chunk's minimum C lies in [LB, U] (every candidate's F is >= the smallest
			// one, L(f) = f - h(f) - e64 is increasing for f >= c^2, c = 1.001 * 64 u M; segments of
			// non-candidate groups are beyond the true minimum or beyond SAT, 6.16^2 = 38).  Both bytes
			// are functions of the bin q = floor(32 sqrt(C) + 1/2) (renderer_precise.rs:71-79: 191 - q
			// outside, 191 + q inside); if the whole interval falls into one bin no f64 work is needed.
			// The reference's own roundings move 32 sqrt(C) by < 1e-12, the f32 evaluation by < 1e-4. ----
			VG_STAMP(7); // phase 2 (pooling + filter rounds)
			bool have = false;
			uint32_t b_in = 255u, b_out = 0u;
			double best = __builtin_huge_val(); // rtree_segments.rs:57
			auto exact_at = [&](double qpx, double qpy, uint32_t i) { // Segment::squared_distance_to_point, from the staged end points
				const double vx = e_vx[i], vy = e_vy[i], wx = e_wx[i], wy = e_wy[i];
				const double dx = wx - vx, dy = wy - vy; // segment.rs:63
				return exact_dist_sq(qpx, qpy, vx, vy, wx, wy, dx, dy, dx * dx + dy * dy);
			};
			bool undecided = false;
			float Tk = __builtin_inff();
			if (!sane) {
				int gx0 = g.x0, gy0 = g.y0;
				asm volatile("" : "+s"(gx0), "+s"(gy0)); // (see the stage: keeps the f64 values out of the kernel-long live ranges)
				const double px = (double)pix_col(rpx, hw) + ((double)gx0 + 0.5), py = (double)(y_hi - roff) + ((double)gy0 + 0.5); // renderer_precise.rs:27-28,34,62
				for (uint32_t j = 0; j < cnt; j++) {
					const double d2 = exact_at(px, py, j);
					best = d2 < best ? d2 : best; // rtree_segments.rs:60-62
				}
				have = true;
			} else if (k1 != 0xFFFFFFFFu) {
				// C lies in [f1 - e, f1 + e], e = h(f1) + e64 (one fused expression; the 1.001 of filter_err covers its
				// roundings).  Bin number of the reference's quantisation: floor(32 sqrt(C) + 1/2).  With 8 e <= f1,
				// |32 sqrt(C) - 32 sqrt(f1)| <= 16.55 e / sqrt(f1) on the whole interval (sqrt is concave: upper side
				// e / (2 sqrt f1), lower side e / (sqrt f1 + sqrt(f1 - e)) <= 1.034 e / (2 sqrt f1)), so if
				// s = 32 sqrt(f1) + 1/2 is farther than dl = 17 e / sqrt(f1) + 3e-4 from the next integer (3e-4: f32
				// roundings of s, < 3e-5, and of the reference's own arithmetic, < 1e-12) every C of the interval
				// falls into bin floor(s).  Beyond C = 35.9 (32 sqrt(C) + 1/2 >= 192) both bytes are saturated (0 / 255)
				// whatever the bin is.  NaN anywhere -> every comparison false -> not decided -> exact evaluation.
				const float f1 = __uint_as_float(k1);
				// (raw v_sqrt_f32: within 1 ulp of the rounded root, which moves s by <= 32 ulp(sq) < 1.6e-5 and e by a 1.2e-7th of its
				// first term, inside the 3e-4 of dl and the 1.001 of h; a denormal f1 gives sq = 0, fails 8 e <= f1 and has dl = inf)
				const float sq = __builtin_amdgcn_sqrtf(f1);
				const float e = VG_M_E(__builtin_fmaf(herr_c1, sq, __builtin_fmaf(VG_HERR_C2S, f1, herr_c3)));
				float U = f1 + e;
				const float uf = U * VG_M_CARRY;
				ub2 = uf < ub2 ? uf : ub2; // bounds the later chunks' candidates too
				const float s = __builtin_fmaf(32.0f, sq, 0.5f);
				const float dl = VG_M_DL(__builtin_fmaf(VG_M_DL_C * e, __builtin_amdgcn_rcpf(sq), VG_M_DL_ABS));
				const float fr = __builtin_amdgcn_fractf(s);
				const float mn = fr < 1.0f - fr ? fr : 1.0f - fr;
				const bool far = f1 - e > VG_M_FAR;
				const bool decided = far || (VG_M_E8(e, f1) && mn > dl);
				if (decided) {
					const int q = far ? 200 : (int)s;
					b_in = (uint32_t)min(191 + q, 255);
					b_out = (uint32_t)max(191 - q, 0);
				} else {
					// Threshold Tk with L(Tk) > U (L increasing above it): fixed-point iteration for the crossing, pushed
					// up, then VERIFIED; if the check fails nothing is excluded (Tk = inf).  Every member of a candidate
					// group whose filter value is at or below Tk is evaluated exactly (below).
					if (!(U >= 0.0f))
						U = __builtin_inff();
					Tk = U + e64;
					for (int it = 0; it < 3; it++)
						Tk = U + e64 + VG_M_E(filter_err(Tk, M));
					Tk = VG_M_TK_PUSH(Tk);
					if (!(Tk - VG_M_E(filter_err(Tk, M)) - e64 > U))
						Tk = __builtin_inff();
					Tk = VG_M_TK(Tk, f1);
					undecided = true;
				}
			}
			VG_STAMP(8); // decide
			// ---- exact evaluation of the undecided pixels, pooled over the wave.  A wave meets an undecided lane in 6 %
			// of its tile-chunks, normally ONE lane; left to itself that lane rescans its candidate groups (8 filter
			// values each) and evaluates the hits in f64 one after the other — ~1400 instructions issued for one lane.
			// Here the wave takes the undecided pixels one at a time and spreads that pixel's (candidate group,
			// member) combinations over its 64 lanes, eight groups per pass: one filter value and at most one f64
			// evaluation per lane, then a minimum over the wave.  The set of segments evaluated (filter value not
			// above Tk) and the f64 operations on each are what the single lane did; min is exact, so is the result. ----
			{
				unsigned long long amb = __ballot(undecided);
				VG_COUNT(cn_fb += amb != 0; cn_fbl += (unsigned long long)__builtin_popcountll(amb);
				         cn_fb_pool += amb != 0 && VG_POOL_MAX != 0 && (uint32_t)__builtin_popcountll(amb) <= (uint32_t)VG_POOL_MAX;
				         cn_fb_lane += amb != 0 && !(VG_POOL_MAX != 0 && (uint32_t)__builtin_popcountll(amb) <= (uint32_t)VG_POOL_MAX));
				if (VG_POOL_MAX != 0 && (uint32_t)__builtin_popcountll(amb) <= (uint32_t)VG_POOL_MAX) {
					while (amb) {
						const int src = (int)__builtin_ctzll(amb);
						amb &= amb - 1;
						const float spx = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(rpx), src));
						const float spy = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(rpy), src));
						const float sTk = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(Tk), src));
						int gx0 = g.x0, gy0 = g.y0;
						asm volatile("" : "+s"(gx0), "+s"(gy0));
						const double dpx = (double)pix_col(spx, hw) + ((double)gx0 + 0.5); // renderer_precise.rs:27-28,34,62
						const double dpy = (double)(y_hi - __builtin_amdgcn_readlane(roff, src)) + ((double)gy0 + 0.5);
						uint32_t scand = (uint32_t)__builtin_amdgcn_readlane((int)cand, src);
						double wbest = __builtin_huge_val();
						while (scand) {
							// lane l looks at member l & 7 of the (l >> 3)-th candidate group still in scand
							uint32_t sel = scand;
							for (uint32_t i = lane >> 3; i != 0; i--)
								sel &= sel - 1;
							if (sel != 0) {
								const uint32_t j = (uint32_t)__builtin_ctz(sel) * GRP + (lane & 7u);
								if (j < cnt && !(sc_filter(spx, spy, s_vx[j], s_vy[j], s_dx[j], s_dy[j], s_inv[j]) > sTk)) {
									const double d2 = exact_at(dpx, dpy, j);
									wbest = d2 < wbest ? d2 : wbest; // rtree_segments.rs:60-62
								}
							}
#pragma unroll
							for (uint32_t i = 0; i < 8; i++)
								scand &= scand - 1; // (wave-uniform: scalar)
						}
						wbest = wave_min_f64(wbest); // (min is exact in any order; wbest is never a NaN)
						if ((int)lane == src)
							best = wbest;
					}
				} else if (undecided) {
					// many undecided lanes (pixels along an edge that sits on a byte boundary): every lane for itself, in parallel
					int gx0 = g.x0, gy0 = g.y0;
					asm volatile("" : "+s"(gx0), "+s"(gy0));
					const double px = (double)pix_col(rpx, hw) + ((double)gx0 + 0.5), py = (double)(y_hi - roff) + ((double)gy0 + 0.5); // renderer_precise.rs:27-28,34,62
					uint32_t m = cand;
					while (m) {
						const uint32_t gq = (uint32_t)__builtin_ctz(m);
						m &= m - 1;
						// members at or below the threshold (padded records have F = 2e36), 4 records at a time
						uint32_t hit = 0;
#pragma unroll 1
						for (uint32_t hq = 0; hq < 2; hq++) {
							const float4 vx4 = q_vx[2 * gq + hq], vy4 = q_vy[2 * gq + hq], dx4 = q_dx[2 * gq + hq], dy4 = q_dy[2 * gq + hq],
							             iv4 = q_inv[2 * gq + hq];
							hit |= !(sc_filter(rpx, rpy, vx4.x, vy4.x, dx4.x, dy4.x, iv4.x) > Tk) ? (1u << (4 * hq)) : 0u;
							hit |= !(sc_filter(rpx, rpy, vx4.y, vy4.y, dx4.y, dy4.y, iv4.y) > Tk) ? (2u << (4 * hq)) : 0u;
							hit |= !(sc_filter(rpx, rpy, vx4.z, vy4.z, dx4.z, dy4.z, iv4.z) > Tk) ? (4u << (4 * hq)) : 0u;
							hit |= !(sc_filter(rpx, rpy, vx4.w, vy4.w, dx4.w, dy4.w, iv4.w) > Tk) ? (8u << (4 * hq)) : 0u;
						}
						while (hit) {
							const uint32_t j = gq * GRP + (uint32_t)__builtin_ctz(hit);
							hit &= hit - 1;
							if (j < cnt) {
								const double d2 = exact_at(px, py, j);
								best = d2 < best ? d2 : best; // rtree_segments.rs:60-62
							}
						}
					}
				}
				have = have || undecided;
			}
			VG_STAMP(9); // exact evaluation (pooled)
			if (have) {
				b_in = quantise(best, true);
				b_out = quantise(best, false);
			}
			// minimum over the chunks, taken on the bytes (monotone in the distance)
			const uint32_t old = st_byte[k * TPB + tid];
			b_in = min(b_in, old & 255u);
			b_out = max(b_out, old >> 8);
			st_byte[k * TPB + tid] = (uint16_t)(b_in | (b_out << 8));
			st_ub2[k * TPB + tid] = ub2;
			VG_STAMP(10); // quantise + state update
		}
	}

	// ---- winding number = prefix sum of the row's histogram up to the pixel's column (renderer_precise.rs:58-66).
	// One thread per row turns its row into inclusive prefix sums in place (exact integer sums, any order);
	// every pixel then reads one cell and picks its byte. ----
	__syncthreads(); // all crossings recorded (n_seg == 0: the initial state / zeroed histogram must be visible)
	{
		const uint32_t n_rows = r_last - r_first + 1;
		for (uint32_t r = tid; r < n_rows; r += TPB) {
			int *drow = s_delta + r * stride;
			int acc = 0;
#pragma unroll 4
			for (uint32_t c = 0; c < g.w; c++) {
				acc += drow[c];
				drow[c] = acc;
			}
		}
	}
	__syncthreads();
	for (uint32_t k = 0; k < T; k++) {
		const uint32_t o = p0 + k * TPB + pw + lane;
		if (o < npix) {
			const uint32_t pe = st_pix[k * TPB + tid]; // (o < npix: the entry is this pixel's own)
			const int wn = s_delta[pix_roff(pe) * stride + (uint32_t)pix_col(pix_rpx(pe), hw)];
			const uint32_t sb = st_byte[k * TPB + tid];
			out[g.out_off + o] = (uint8_t)(wn != 0 ? (sb & 255u) : (sb >> 8));
		}
	}
	VG_STAMP(11); // epilogue: winding prefix sums, stores
#if defined(VG_SPAN_STAMPED) || defined(VG_SPAN_COUNTED)
	if (lane == 0) {
#ifdef VG_SPAN_STAMPED
		for (int r = 0; r < 12; r++)
			atomicAdd(&g_span_dbg[r], st_acc[r]);
#endif
		atomicAdd(&g_span_dbg[12], 1ull);
		atomicAdd(&g_span_dbg[13], cn_pairs);
		atomicAdd(&g_span_dbg[14], cn_rounds);
		atomicAdd(&g_span_dbg[15], cn_tc);
		atomicAdd(&g_span_dbg[16], cn_fb);
		atomicAdd(&g_span_dbg[17], cn_fbl);
		atomicAdd(&g_span_dbg[20], cn_over);
		atomicAdd(&g_span_dbg[21], cn_fb_pool);
		atomicAdd(&g_span_dbg[22], cn_fb_lane);
		atomicAdd(&g_span_dbg[23], cn_half);
		atomicAdd(&g_span_dbg[24], cn_leave);
		atomicAdd(&g_span_dbg[25], cn_row_fb);
	}
#endif
}

#undef VG_SPAN_KERNEL
#undef VG_STAMP
#undef VG_COUNT
// one #undef per VG_M_* macro defined at the top of this file (keep the two lists in step: a macro left defined would
// carry one stamping's override into the next; the VG_HERR_* / VG_E64_C constants of sdf_span_support.h are per file, not
// per stamping).  Not every name has an instance that overrides it: the names are the inventory of DESIGN.md §4.1.
#undef VG_M_BOX_PADK
#undef VG_M_BOX_SAT
#undef VG_M_BOX_R
#undef VG_M_BOX_BAND
#undef VG_M_INFL
#undef VG_M_GRP_SLACK
#undef VG_M_PAD
#undef VG_M_RG
#undef VG_M_SAT
#undef VG_M_SANE
#undef VG_M_BOUNDED
#undef VG_M_MABS0
#undef VG_M_E64
#undef VG_M_E
#undef VG_M_CARRY
#undef VG_M_DL
#undef VG_M_DL_C
#undef VG_M_DL_ABS
#undef VG_M_E8
#undef VG_M_FAR
#undef VG_M_TK_PUSH
#undef VG_M_TK
#undef VG_M_ROW_E
