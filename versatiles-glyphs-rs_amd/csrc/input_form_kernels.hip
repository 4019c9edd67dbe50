// input_form_kernels.hip — how a submission's commands come to be on the device, one kernel per input form: the `glyf`
// decoder (stamped for bytes of the submission and for bytes of resident fonts), copy_in (a page-locked block), resident_expand /
// resident_gather (glyphs named against resident glyf / command fonts), family_expand / family_gather (code-point ranges of
// resident families).  What they leave — OutlineCmd records, and where they can the context bytes — is what the flattening
// pipeline (outline_kernels.hip) reads.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "input_form_kernels.h"
#include "upload_layout.h"
#include "wave_ops.h"

namespace vgsdf {

// ---------------------------------------------------------------------------------------
// glyf decode: thread per PART (one simple glyph of a — possibly composite — glyph, with the transform ttf-parser has
// accumulated for it).  The host only looks glyphs up and copies each simple glyph's `glyf` arrays (end points of the
// contours, then flags / x / y as they stand in the font, instructions left out); this pass replays ttf-parser's walk
// (glyf.rs: parse_simple_outline — flag runs, short / same-or-positive coordinates, wrapping i16 sums — and Builder:
// implied on-curve midpoints, the closing curve of a contour, close()) and writes the OutlineBuilder callbacks as the
// OutlineCmd records every later pass reads: what csrc/host/ttf_face.cpp records on the host, callback for callback
// (f32, one multiply-add pair per transformed coordinate, never fused).
// A part owns `cmd_cap` >= points + 2 * contours command slots (a contour of L points brings at most L + 2 callbacks: one per
// point, the closing line or curve, close(); the second closing curve of a contour that begins and ends off the curve comes
// instead of its first point's callback; end points that do not ascend cannot add contours — the lengths EndpointsIter
// hands out sum to at least the point count); the slots it does not need are filled with close():
// on the empty ring that follows a contour's own close() the RingBuilder does nothing (ring_builder.rs:33-38).
// error_flag bit 4: an entry whose arrays do not fit its bytes or its slots — ttf-parser would drop that glyph and, in a
// composite, the components after it; the host records such a batch itself.
// ---------------------------------------------------------------------------------------
struct GlyfPart {          // mirrors vgsdf_glyf_part (include/vgsdf.h)
	uint32_t byte_off;     // into `bytes`: endPtsOfContours[n_contours], then the flag / x / y arrays of the entry
	uint32_t byte_len;
	uint32_t cmd_at, cmd_cap;
	uint32_t n_contours;
	uint32_t plain;        // 1: identity transform
	float a, b, c, d, e, f;
};
static_assert(sizeof(GlyfPart) == 48, "GlyfPart layout");

// One wave per part, the points dealt out to the lanes (a lane that walks a 300-point glyph alone needs ~0.2 ms: ~700 dependent
// instructions per point on a machine that issues one every few cycles per wave):
//   A  flags: run-length decoding without a walk.  A byte of the flag stream is a repeat COUNT iff the byte in front of it
//      is a flag with REPEAT set — inside a run of bytes that all carry bit 3 flags and counts alternate, so a byte's role
//      follows from the length of the run of such bytes in front of it (one ballot per 64 bytes); runs are laid out by a
//      prefix sum, every flag lands on the points it covers (LDS), the sizes of the x / y arrays come out as sums.
//   B  coordinates: offset of a point's delta = prefix sum of the sizes its flags give, value = prefix sum of the deltas
//      (mod 2^16, as the i16 additions of the walk wrap).
//   C  contours and callbacks: the end points give every contour's first and last point (ttf-parser's EndpointsIter, also for
//      end points that do not ascend); what Builder::push_point emits for a point depends on its own flag, the flag of
//      the point in front of it and the first two points of its contour — no state is carried; the last point of a
//      contour also emits what Builder::finish adds; positions by prefix sum.
// A wave's time is a handful of dependent memory round trips (~1.5 us each), not arithmetic: the part's bytes are fetched
// ONCE (coalesced dwords into LDS; flags, coordinates and end points are then read there), and the LDS a workgroup takes is
// sized per launch from the batch's largest part, so that as a rule every part of a font is resident at once (3993 parts of
// Noto Sans Regular: 25.8 us with 21 KB of LDS per wave and the arrays read from global memory).
constexpr uint32_t kGlyfMaxPoints = 6144; // per part (LDS: 1 + 2 + 2 bytes per point + its bytes); beyond: the host's reader (error_flag bit 4)
constexpr uint32_t kGlyfMaxBytes = 30 * 1024;   // (together below the 64 KB a workgroup gets without asking for more)

// max_points / max_bytes: what the launch's LDS was sized for (the batch's largest cmd_cap bounds its largest point count)
// cmd_open (may be NULL): the context pass's result for these commands, written here as well — whether the ring is non-empty in
// front of a command follows from the contour rules alone: every contour of a part begins on an empty ring (the contour
// in front of it, or the filler behind the previous part, ended with close()), its move_to opens the ring and everything
// behind it up to its close() finds it open.  (Bit 1 of the context byte — a glyph whose scale is not positive and finite —
// is the caller's to rule out: the host passes cmd_open only when every scale of the batch is.)
#define GLYF_DECODE_RESIDENT 0
#include "glyf_decode_kernel.inc"
#undef GLYF_DECODE_RESIDENT
#define GLYF_DECODE_RESIDENT 1
#include "glyf_decode_kernel.inc"
#undef GLYF_DECODE_RESIDENT

// The upload of a submission whose input sits in ONE page-locked, device-mapped block: 16 bytes per thread, every load of
// the block in flight at once — one PCIe round trip plus the bytes, without the copy engine's hand-over in front of the
// first kernel (hipMemcpyAsync: 16.5 us for the 200 KB of a font + 8.7 us until the next kernel starts).
__global__ __launch_bounds__(256) void copy_in(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16, const uint8_t *__restrict__ src_tail,
                                               uint8_t *__restrict__ dst_tail, uint32_t n_tail)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n16)
		dst[i] = src[i];
	if (i < n_tail)
		dst_tail[i] = src_tail[i];
}

// The upload of a submission that names its glyphs (vgsdf_outlines_resident): copy_in's copy of the ONE page-locked block
// (upload_layout.h, ResidentBlockLayout: per-glyph arrays + the fonts' device addresses), and the expansion of the glyphs'
// leaves into this submission's parts.  A workgroup takes 256 glyphs: their offsets, glyph ids and font indices go to LDS
// with the same round trip as the copy's loads, then the LEAVES of those glyphs — [part_off[g0], part_off[g0 + 256)) — are
// dealt to the lanes one each (1.3 - 1.5 per glyph with a long tail: a composite of composites does not hold a lane back);
// a lane finds its leaf's glyph by bisection in LDS, reads the leaf from the resident table of the glyph's font (HBM) and
// stores it as part part_off[g] + k with cmd_at moved to the glyph's slots and the font's index beside `plain`.
constexpr uint32_t kExpandThreads = 256, kExpandFontCache = 128;
__global__ __launch_bounds__(kExpandThreads) void resident_expand(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16,
                                                                  uint32_t n_glyphs, uint32_t n_parts, uint32_t n_fonts, uint32_t cmd_off_at,
                                                                  uint32_t part_off_at, uint32_t glyph_id_at, uint32_t font_of_at,
                                                                  uint32_t fonts_at, GlyfPart *__restrict__ parts_out)
{
	__shared__ uint32_t s_part_off[kExpandThreads + 1], s_cmd_off[kExpandThreads];
	__shared__ uint16_t s_gid[kExpandThreads], s_font[kExpandThreads];
	__shared__ ResidentFontRef s_fonts[kExpandFontCache];
	const uint32_t t = threadIdx.x, i = blockIdx.x * kExpandThreads + t, g0 = blockIdx.x * kExpandThreads;
	const uint8_t *const sb = reinterpret_cast<const uint8_t *>(src);
	const ResidentFontRef *const fonts = reinterpret_cast<const ResidentFontRef *>(sb + fonts_at);
	uint4 v = make_uint4(0, 0, 0, 0);
	if (i < n16)
		v = src[i];
	const uint32_t ng = g0 < n_glyphs ? min(kExpandThreads, n_glyphs - g0) : 0u;
	if (ng) {
		const uint32_t *part_off = reinterpret_cast<const uint32_t *>(sb + part_off_at) + g0;
		for (uint32_t k = t; k <= ng; k += kExpandThreads)
			s_part_off[k] = part_off[k];
		if (t < ng) {
			s_cmd_off[t] = reinterpret_cast<const uint32_t *>(sb + cmd_off_at)[g0 + t];
			s_gid[t] = reinterpret_cast<const uint16_t *>(sb + glyph_id_at)[g0 + t];
			s_font[t] = reinterpret_cast<const uint16_t *>(sb + font_of_at)[g0 + t];
		}
		for (uint32_t k = t; k < min(n_fonts, kExpandFontCache); k += kExpandThreads)
			s_fonts[k] = fonts[k];
	}
	if (i < n16)
		dst[i] = v;
	if (ng == 0) // (uniform in the workgroup)
		return;
	__syncthreads();
#include "resident_expand_leaves.inc"
}

// The upload of a submission that names its glyphs against COMMAND fonts (vgsdf_font_create_commands): copy_in's copy of the
// ONE page-locked block (upload_layout.h, CommandBlockLayout) and the gather of every named glyph's expanded records and
// context bytes from its font's store into the batch's command arrays at cmd_off[g] — a pure segmented copy: no decoder and,
// when every scale is positive and finite, no context pass runs behind it.  A workgroup takes 256 glyphs as resident_expand
// does: lane t reads glyph g0 + t's offset, id and font index with the same round trip as the copy's loads (and the font
// references go to LDS), looks its glyph's first record up in the font's offset table and leaves the two source addresses in
// LDS; then the COMMANDS of those glyphs — [cmd_off[g0], cmd_off[g0 + 256)) — are dealt to the lanes, kGatherUnroll per lane
// and round with every load of a round in flight before its first store (a 5000-command glyph holds no lane back), and a
// lane finds its command's glyph by bisection in LDS.  Records are 4-byte aligned only (28 bytes: seven dword copies); the
// context bytes start at any byte offset on either side and travel a byte per lane.
constexpr uint32_t kGatherUnroll = 4;
__global__ __launch_bounds__(kExpandThreads) void resident_gather(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16,
                                                                  uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_fonts, uint32_t cmd_off_at,
                                                                  uint32_t glyph_id_at, uint32_t font_of_at, uint32_t fonts_at,
                                                                  uint32_t *__restrict__ cmds_out, uint8_t *__restrict__ open_out)
{
	__shared__ uint32_t s_cmd_off[kExpandThreads + 1];
	__shared__ const uint32_t *s_recs[kExpandThreads];
	__shared__ const uint8_t *s_open[kExpandThreads];
	__shared__ CommandFontRef s_fonts[kExpandFontCache];
	const uint32_t t = threadIdx.x, i = blockIdx.x * kExpandThreads + t, g0 = blockIdx.x * kExpandThreads;
	const uint8_t *const sb = reinterpret_cast<const uint8_t *>(src);
	const CommandFontRef *const fonts = reinterpret_cast<const CommandFontRef *>(sb + fonts_at);
	uint4 v = make_uint4(0, 0, 0, 0);
	if (i < n16)
		v = src[i];
	const uint32_t ng = g0 < n_glyphs ? min(kExpandThreads, n_glyphs - g0) : 0u;
	uint32_t gid = 0, f = 0;
	if (ng) {
		const uint32_t *cmd_off = reinterpret_cast<const uint32_t *>(sb + cmd_off_at) + g0;
		for (uint32_t k = t; k <= ng; k += kExpandThreads)
			s_cmd_off[k] = cmd_off[k];
		if (t < ng) {
			gid = reinterpret_cast<const uint16_t *>(sb + glyph_id_at)[g0 + t];
			f = reinterpret_cast<const uint16_t *>(sb + font_of_at)[g0 + t];
		}
		for (uint32_t k = t; k < min(n_fonts, kExpandFontCache); k += kExpandThreads)
			s_fonts[k] = fonts[k];
	}
	if (i < n16)
		dst[i] = v;
	if (ng == 0) // (uniform in the workgroup)
		return;
	__syncthreads();
#include "resident_gather_records.inc"
}

// The upload of a submission that names its glyphs against fonts of BOTH kinds in one list (vgsdf_outlines_submit_resident_mixed):
// the block is ResidentBlockLayout's, part_off standing still over a glyph of a command font and cmd_off running over the glyphs of
// both kinds, and every font reference says its kind (upload_layout.h, MixedFontRef).  One launch of 256 glyphs per workgroup as
// the two kernels above, one LDS cache of kExpandFontCache references, and BOTH second phases: the leaves of the workgroup's
// glyf glyphs become parts, the records and context bytes of its command glyphs are gathered.  The gather's range
// [cmd_off[g0], cmd_off[g0 + 256)) spans the slots of the workgroup's glyf glyphs as well: those it passes over — the decoder,
// which runs behind this kernel over the parts, fills them.
__global__ __launch_bounds__(kExpandThreads) void resident_mixed(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16,
                                                                 uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_parts, uint32_t n_fonts,
                                                                 uint32_t cmd_off_at, uint32_t part_off_at, uint32_t glyph_id_at,
                                                                 uint32_t font_of_at, uint32_t fonts_at, GlyfPart *__restrict__ parts_out,
                                                                 uint32_t *__restrict__ cmds_out, uint8_t *__restrict__ open_out)
{
	__shared__ uint32_t s_part_off[kExpandThreads + 1], s_cmd_off[kExpandThreads + 1];
	__shared__ uint16_t s_gid[kExpandThreads], s_font[kExpandThreads];
	__shared__ const uint32_t *s_recs[kExpandThreads];
	__shared__ const uint8_t *s_open[kExpandThreads];
	__shared__ MixedFontRef s_fonts[kExpandFontCache];
	const uint32_t t = threadIdx.x, i = blockIdx.x * kExpandThreads + t, g0 = blockIdx.x * kExpandThreads;
	const uint8_t *const sb = reinterpret_cast<const uint8_t *>(src);
	const MixedFontRef *const fonts = reinterpret_cast<const MixedFontRef *>(sb + fonts_at);
	uint4 v = make_uint4(0, 0, 0, 0);
	if (i < n16)
		v = src[i];
	const uint32_t ng = g0 < n_glyphs ? min(kExpandThreads, n_glyphs - g0) : 0u;
	uint32_t gid = 0, f = 0;
	if (ng) {
		const uint32_t *part_off = reinterpret_cast<const uint32_t *>(sb + part_off_at) + g0;
		const uint32_t *cmd_off = reinterpret_cast<const uint32_t *>(sb + cmd_off_at) + g0;
		for (uint32_t k = t; k <= ng; k += kExpandThreads) {
			s_part_off[k] = part_off[k];
			s_cmd_off[k] = cmd_off[k];
		}
		if (t < ng) {
			gid = reinterpret_cast<const uint16_t *>(sb + glyph_id_at)[g0 + t];
			f = reinterpret_cast<const uint16_t *>(sb + font_of_at)[g0 + t];
			s_gid[t] = (uint16_t)gid;
			s_font[t] = (uint16_t)f;
		}
		for (uint32_t k = t; k < min(n_fonts, kExpandFontCache); k += kExpandThreads)
			s_fonts[k] = fonts[k];
	}
	if (i < n16)
		dst[i] = v;
	if (ng == 0) // (uniform in the workgroup)
		return;
	__syncthreads();
	{
#include "resident_expand_leaves.inc"
	}
#define RESIDENT_GATHER_MIXED
#include "resident_gather_records.inc"
#undef RESIDENT_GATHER_MIXED
}

// The uploads of a submission that names code-point ranges of resident families: what the launch is given (the counts every
// index of the block is bounded against, where the block's records lie, where the device's copy has its per-glyph arrays)
constexpr uint32_t kFamilyCache = 64; // family records a workgroup keeps in LDS
struct FamilyLaunch {
	uint32_t n_glyphs, n_cmds, n_parts, n_fonts, n_tasks, n_families, with_pbf;
	uint32_t families_at, fonts_at; // in the block (its task records begin it)
	uint32_t d_scale, d_shift_x, d_cmd_off, d_part_off, d_glyph_id, d_font_of, d_pbf_pre, d_pbf_fix, d_fonts; // in the device's copy
};
#define FAMILY_GLYF 1
#include "family_upload_kernel.inc"
#undef FAMILY_GLYF
#define FAMILY_GLYF 0
#include "family_upload_kernel.inc"
#undef FAMILY_GLYF
#define FAMILY_MIXED
#define RESIDENT_GATHER_MIXED
#include "family_upload_kernel.inc"
#undef RESIDENT_GATHER_MIXED
#undef FAMILY_MIXED

} // namespace vgsdf

using namespace vgsdf;

extern "C" int vgsdf_resident_gather(const void *src, void *dst, size_t block_bytes, uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_fonts,
                                     bool with_pbf, OutlineCmd *cmds_out, uint8_t *cmd_open, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	const CommandBlockLayout cl(n_glyphs, n_fonts, with_pbf);
	const uint32_t n16 = (uint32_t)((block_bytes + 15) / 16); // (the block and its device copy are padded to 16 bytes)
	const uint32_t grid = (std::max(n16, n_glyphs) + kExpandThreads - 1u) / kExpandThreads;
	hipLaunchKernelGGL(resident_gather, dim3(grid), dim3(kExpandThreads), 0, stream, (const uint4 *)src, (uint4 *)dst, n16, n_glyphs, n_cmds,
	                   n_fonts, (uint32_t)cl.cmd_off, (uint32_t)cl.glyph_id, (uint32_t)cl.font_of, (uint32_t)cl.fonts, (uint32_t *)cmds_out,
	                   cmd_open);
	return (int)hipGetLastError();
}

extern "C" void vgsdf_glyf_limits(uint32_t *max_points, uint32_t *max_bytes, uint32_t *expand_font_cache)
{
	if (max_points)
		*max_points = kGlyfMaxPoints;
	if (max_bytes)
		*max_bytes = kGlyfMaxBytes;
	if (expand_font_cache)
		*expand_font_cache = kExpandFontCache;
}

extern "C" int vgsdf_resident_expand(const void *src, void *dst, size_t block_bytes, uint32_t n_glyphs, uint32_t n_parts, uint32_t n_fonts,
                                     bool with_pbf, void *parts_out, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	const ResidentBlockLayout rl(n_glyphs, n_fonts, with_pbf);
	const uint32_t n16 = (uint32_t)((block_bytes + 15) / 16); // (the block and its device copy are padded to 16 bytes)
	const uint32_t grid = (std::max(n16, n_glyphs) + kExpandThreads - 1u) / kExpandThreads;
	hipLaunchKernelGGL(resident_expand, dim3(grid), dim3(kExpandThreads), 0, stream, (const uint4 *)src, (uint4 *)dst, n16, n_glyphs, n_parts,
	                   n_fonts, (uint32_t)rl.cmd_off, (uint32_t)rl.part_off, (uint32_t)rl.glyph_id, (uint32_t)rl.font_of, (uint32_t)rl.fonts,
	                   (GlyfPart *)parts_out);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_resident_mixed(const void *src, void *dst, size_t block_bytes, uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_parts,
                                    uint32_t n_fonts, bool with_pbf, void *parts_out, OutlineCmd *cmds_out, uint8_t *cmd_open, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	const ResidentBlockLayout rl(n_glyphs, n_fonts, with_pbf);
	const uint32_t n16 = (uint32_t)((block_bytes + 15) / 16); // (the block and its device copy are padded to 16 bytes)
	const uint32_t grid = (std::max(n16, n_glyphs) + kExpandThreads - 1u) / kExpandThreads;
	hipLaunchKernelGGL(resident_mixed, dim3(grid), dim3(kExpandThreads), 0, stream, (const uint4 *)src, (uint4 *)dst, n16, n_glyphs, n_cmds,
	                   n_parts, n_fonts, (uint32_t)rl.cmd_off, (uint32_t)rl.part_off, (uint32_t)rl.glyph_id, (uint32_t)rl.font_of,
	                   (uint32_t)rl.fonts, (GlyfPart *)parts_out, (uint32_t *)cmds_out, cmd_open);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_family_upload(int kind, const void *src, void *dst, uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_parts,
                                   uint32_t n_fonts, uint32_t n_tasks, uint32_t n_families, bool with_pbf, void *parts_out,
                                   OutlineCmd *cmds_out, uint8_t *cmd_open, void *names, uint32_t *error_flag, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	const RangesBlockLayout bl(n_tasks, n_families, n_fonts);
	FamilyLaunch L{};
	L.n_glyphs = n_glyphs, L.n_cmds = n_cmds, L.n_parts = n_parts, L.n_fonts = n_fonts, L.n_tasks = n_tasks, L.n_families = n_families;
	L.with_pbf = with_pbf ? 1u : 0u;
	L.families_at = (uint32_t)bl.families, L.fonts_at = (uint32_t)bl.fonts;
	const uint32_t grid = (std::max(n_glyphs, 2u * n_fonts) + kExpandThreads - 1u) / kExpandThreads;
	if (kind == VGSDF_FONTS_COMMANDS) {
		const CommandBlockLayout cl(n_glyphs, n_fonts, with_pbf);
		L.d_scale = (uint32_t)cl.scale, L.d_shift_x = (uint32_t)cl.shift_x, L.d_cmd_off = (uint32_t)cl.cmd_off;
		L.d_glyph_id = (uint32_t)cl.glyph_id, L.d_font_of = (uint32_t)cl.font_of, L.d_pbf_pre = (uint32_t)cl.pbf_pre;
		L.d_pbf_fix = (uint32_t)cl.pbf_fix, L.d_fonts = (uint32_t)cl.fonts;
		hipLaunchKernelGGL(family_gather, dim3(grid), dim3(kExpandThreads), 0, stream, (const uint8_t *)src, (uint8_t *)dst, L,
		                   (uint32_t *)cmds_out, cmd_open, (EntryName *)names, error_flag);
	} else {
		const ResidentBlockLayout rl(n_glyphs, n_fonts, with_pbf);
		L.d_scale = (uint32_t)rl.scale, L.d_shift_x = (uint32_t)rl.shift_x, L.d_cmd_off = (uint32_t)rl.cmd_off, L.d_part_off = (uint32_t)rl.part_off;
		L.d_glyph_id = (uint32_t)rl.glyph_id, L.d_font_of = (uint32_t)rl.font_of, L.d_pbf_pre = (uint32_t)rl.pbf_pre;
		L.d_pbf_fix = (uint32_t)rl.pbf_fix, L.d_fonts = (uint32_t)rl.fonts;
		if (kind == VGSDF_FONTS_MIXED)
			hipLaunchKernelGGL(family_mixed, dim3(grid), dim3(kExpandThreads), 0, stream, (const uint8_t *)src, (uint8_t *)dst, L,
			                   (GlyfPart *)parts_out, (uint32_t *)cmds_out, cmd_open, (EntryName *)names, error_flag);
		else
			hipLaunchKernelGGL(family_expand, dim3(grid), dim3(kExpandThreads), 0, stream, (const uint8_t *)src, (uint8_t *)dst, L,
			                   (GlyfPart *)parts_out, (EntryName *)names, error_flag);
	}
	return (int)hipGetLastError();
}

extern "C" int vgsdf_copy_in(const void *src_mapped, void *dst, size_t bytes, hipStream_t stream)
{
	if (bytes == 0)
		return 0;
	const uint32_t n16 = (uint32_t)(bytes / 16), n_tail = (uint32_t)(bytes % 16);
	hipLaunchKernelGGL(copy_in, dim3((std::max(n16, 1u) + 255u) / 256u), dim3(256), 0, stream, (const uint4 *)src_mapped, (uint4 *)dst, n16,
	                   (const uint8_t *)src_mapped + 16 * (size_t)n16, (uint8_t *)dst + 16 * (size_t)n16, n_tail);
	return (int)hipGetLastError();
}

// LDS of a workgroup of the glyf decoder (either stamping): the largest part's bytes + 5 bytes and a bit per point (a part has
// fewer points than command slots); parts beyond the limits fail on the device (error_flag bit 4: the host's reader takes the
// batch).  Sets the two bounds the kernel is launched with
static size_t glyf_decode_lds(uint32_t max_cmd_cap, uint32_t max_byte_len, uint32_t &max_points, uint32_t &max_bytes)
{
	max_points = std::min(std::max(max_cmd_cap, 64u), kGlyfMaxPoints);
	max_bytes = std::min((std::max(max_byte_len, 64u) + 15u) & ~15u, kGlyfMaxBytes);
	return (size_t)max_bytes + 4 * (size_t)max_points + 4 * (size_t)((max_points + 31u) / 32u) + max_points;
}

extern "C" int vgsdf_glyf_decode(const void *parts, uint32_t n_parts, const uint8_t *bytes, OutlineCmd *cmds, uint32_t *error_flag,
                                 uint32_t max_cmd_cap, uint32_t max_byte_len, uint8_t *cmd_open, hipStream_t stream)
{
	if (n_parts == 0)
		return 0;
	uint32_t max_points, max_bytes;
	const size_t lds = glyf_decode_lds(max_cmd_cap, max_byte_len, max_points, max_bytes);
	hipLaunchKernelGGL(glyf_decode, dim3(n_parts), dim3(64), lds, stream, (const GlyfPart *)parts, n_parts, bytes, cmds, error_flag, max_points,
	                   max_bytes, cmd_open);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_glyf_decode_resident(const void *parts, uint32_t n_parts, const void *fonts, OutlineCmd *cmds, uint32_t *error_flag,
                                          uint32_t max_cmd_cap, uint32_t max_byte_len, uint8_t *cmd_open, hipStream_t stream)
{
	if (n_parts == 0)
		return 0;
	uint32_t max_points, max_bytes;
	const size_t lds = glyf_decode_lds(max_cmd_cap, max_byte_len, max_points, max_bytes);
	hipLaunchKernelGGL(glyf_decode_resident, dim3(n_parts), dim3(64), lds, stream, (const GlyfPart *)parts, n_parts,
	                   (const ResidentFontRef *)fonts, cmds, error_flag, max_points, max_bytes, cmd_open);
	return (int)hipGetLastError();
}
