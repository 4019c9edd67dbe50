// family_upload_kernel.inc — the upload kernel of a submission that names code-point RANGES of resident families
// (vgsdf_outlines_ranges), stamped once per kind of font by input_form_kernels.hip:
//   FAMILY_GLYF 1  family_expand   fonts from vgsdf_font_create: takes resident_expand's place
//   FAMILY_GLYF 0  family_gather   fonts from vgsdf_font_create_commands: takes resident_gather's place
//   FAMILY_MIXED   family_mixed    mixed families, fonts of both kinds in one list (upload_layout.h, MixedFontRef): takes
//                                  resident_mixed's place — the per-glyph arrays of ResidentBlockLayout with no parts for an
//                                  entry of a command font, then BOTH second phases
// The block (upload_layout.h, RangesBlockLayout) holds a record per task, per family and per font and NOTHING per glyph: the
// naming — task -> family entry -> (font, glyph id, scale, shift, offsets) — happens here, in front of the expansion / gather
// the kernel would run anyway, so the form adds no launch.  A workgroup takes 256 glyphs of the submission, as those kernels
// do.  The first task that reaches into them is found by a bisection every lane runs alike over the block's task records
// (uniform addresses); tasks that map nothing are not in the block, so at most 256 tasks overlap the workgroup and their
// records go to LDS with one load per lane, beside the first family and font references.  Lane t then bisects those records
// for glyph g0 + t's task, reads its entry of the family's device table and the two prefix sums, and WRITES the per-glyph
// arrays of ResidentBlockLayout / CommandBlockLayout into the block's device copy, exactly where every later kernel reads
// them — cmd_off[n] and part_off[n] by the lane of the last glyph alone — and, for in-place PBF assembly, the id and
// advance pbf_entries needs.  What the second phase needs stays in LDS, and that phase is the text of the kernel whose place this
// one takes (resident_expand_leaves.inc / resident_gather_records.inc).
// Every index that comes from the block is bounded against what the launch was given (task and family counts, the family's
// entry count, the font count, n_cmds, n_parts) before it is followed; a bad one raises bit 5 of the batch's error word, its
// glyph is named as a glyph without outline and the workgroup, instead of expanding / gathering, makes every part / record of
// the submission a benign one (below).
#if defined(FAMILY_MIXED)
#define FAMILY_KERNEL family_mixed
#define FAMILY_FONT_REF MixedFontRef
#define FAMILY_PARTS 1
#define FAMILY_RECORDS 1
#elif FAMILY_GLYF
#define FAMILY_KERNEL family_expand
#define FAMILY_FONT_REF ResidentFontRef
#define FAMILY_PARTS 1
#define FAMILY_RECORDS 0
#else
#define FAMILY_KERNEL family_gather
#define FAMILY_FONT_REF CommandFontRef
#define FAMILY_PARTS 0
#define FAMILY_RECORDS 1
#endif
__global__ __launch_bounds__(kExpandThreads) void FAMILY_KERNEL(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const FamilyLaunch L,
#if FAMILY_PARTS
                                                                GlyfPart *__restrict__ parts_out,
#endif
#if FAMILY_RECORDS
                                                                uint32_t *__restrict__ cmds_out, uint8_t *__restrict__ open_out,
#endif
                                                                EntryName *__restrict__ names, uint32_t *__restrict__ error_flag)
{
	__shared__ RangeTask s_task[kExpandThreads];
	__shared__ FamilyRef s_fam[kFamilyCache];
	__shared__ FAMILY_FONT_REF s_fonts[kExpandFontCache];
#if FAMILY_PARTS
	__shared__ uint32_t s_part_off[kExpandThreads + 1], s_cmd_off[kExpandThreads + FAMILY_RECORDS];
	__shared__ uint16_t s_gid[kExpandThreads], s_font[kExpandThreads];
	const uint32_t n_parts = L.n_parts;
#else
	__shared__ uint32_t s_cmd_off[kExpandThreads + 1];
#endif
#if FAMILY_RECORDS
	__shared__ const uint32_t *s_recs[kExpandThreads];
	__shared__ const uint8_t *s_open[kExpandThreads];
#endif
	const uint32_t n_cmds = L.n_cmds, n_fonts = L.n_fonts;
	const uint32_t t = threadIdx.x, i = blockIdx.x * kExpandThreads + t, g0 = blockIdx.x * kExpandThreads;
	const RangeTask *const tasks = reinterpret_cast<const RangeTask *>(src);
	const FamilyRef *const fams = reinterpret_cast<const FamilyRef *>(src + L.families_at);
	const FAMILY_FONT_REF *const fonts = reinterpret_cast<const FAMILY_FONT_REF *>(src + L.fonts_at);
	// the font references travel as they stand: the decoder reads them from the device's copy (two 16-byte halves each)
	if (i < 2u * n_fonts)
		reinterpret_cast<uint4 *>(dst + L.d_fonts)[i] = reinterpret_cast<const uint4 *>(src + L.fonts_at)[i];
	const uint32_t ng = g0 < L.n_glyphs ? min(kExpandThreads, L.n_glyphs - g0) : 0u;
	if (ng == 0 || L.n_tasks == 0) // (uniform in the workgroup)
		return;
	// the last task that begins at or in front of glyph g0: the same walk in every lane
	uint32_t t0 = 0;
	for (uint32_t hi = L.n_tasks; hi - t0 > 1u;) {
		const uint32_t mid = (t0 + hi) >> 1;
		if (tasks[mid].glyph_base <= g0)
			t0 = mid;
		else
			hi = mid;
	}
	const uint32_t nt = min(kExpandThreads, L.n_tasks - t0);
	if (t < nt) {
		const uint4 *tp = reinterpret_cast<const uint4 *>(tasks + t0 + t);
		uint4 *sp = reinterpret_cast<uint4 *>(&s_task[t]);
		sp[0] = tp[0];
		sp[1] = tp[1];
	}
	for (uint32_t k = t; k < min(L.n_families, kFamilyCache); k += kExpandThreads)
		s_fam[k] = fams[k];
	for (uint32_t k = t; k < min(n_fonts, kExpandFontCache); k += kExpandThreads)
		s_fonts[k] = fonts[k];
	__syncthreads();
	uint32_t gid = 0, f = 0;
	bool bad = false;
	if (t < ng) {
		const uint32_t g = g0 + t;
		uint32_t lo = 0;
		for (uint32_t hi = nt; hi - lo > 1u;) {
			const uint32_t mid = (lo + hi) >> 1;
			if (s_task[mid].glyph_base <= g)
				lo = mid;
			else
				hi = mid;
		}
		const RangeTask T = s_task[lo];
		const uint32_t k = g - T.glyph_base;
		// a glyph without outline at the end of everything: what a lane names whose indices do not hold
		uint32_t cmd_at = n_cmds, cmd_n = 0, pre = 0, fix = 0x22u;
#if FAMILY_PARTS
		uint32_t part_at = n_parts, part_n = 0;
#endif
		double scale = 1.0, shift = 0.0;
		EntryName nm = {0u, 0u, 0u, 0u};
		bad = T.glyph_base > g || k >= T.n_glyphs || T.family >= L.n_families;
		if (!bad) {
			const FamilyRef F = T.family < kFamilyCache ? s_fam[T.family] : fams[T.family];
			const unsigned long long e = (unsigned long long)T.entry_first + k;
			bad = e >= F.n_entries || F.n_entries > 0x10000u || (unsigned long long)F.font_base + F.n_fonts > n_fonts;
			if (!bad) {
				const FamilyTableLayout at(F.n_entries);
				const uint8_t *const tb = reinterpret_cast<const uint8_t *>(F.table);
				const uint32_t *const cp = reinterpret_cast<const uint32_t *>(tb + at.cmd_pre) + e;
				const uint32_t c0 = cp[0], c1 = cp[1];
				const uint32_t fo = reinterpret_cast<const uint16_t *>(tb + at.font_of)[e];
				cmd_at = T.cmd_rel + c0;
				cmd_n = c1 - c0;
				bad = fo >= F.n_fonts || (unsigned long long)cmd_at + cmd_n > n_cmds;
#if FAMILY_PARTS
				const uint32_t *const lp = reinterpret_cast<const uint32_t *>(tb + at.leaf_pre) + e;
				const uint32_t l0 = lp[0], l1 = lp[1];
				part_at = T.part_rel + l0;
				part_n = l1 - l0;
				bad = bad || (unsigned long long)part_at + part_n > n_parts;
#endif
				if (!bad) {
					f = F.font_base + fo;
					gid = reinterpret_cast<const uint16_t *>(tb + at.glyph_id)[e];
					scale = reinterpret_cast<const double *>(tb + at.scale)[e];
					shift = reinterpret_cast<const double *>(tb + at.shift_x)[e];
					if (L.with_pbf) {
						pre = k == 0 ? T.pbf_pre : 0u;
						fix = (tb + at.pbf_fix)[e];
						nm.id = F.cp_base + reinterpret_cast<const uint16_t *>(tb + at.code_point)[e];
						nm.advance = reinterpret_cast<const uint32_t *>(tb + at.advance)[e];
						nm.task_first = k == 0 ? t0 + lo + 1u : 0u;
					}
				}
			}
		}
		if (bad) {
			atomicOr(error_flag, 32u);
			cmd_at = n_cmds, cmd_n = 0;
#if FAMILY_PARTS
			part_at = n_parts, part_n = 0;
#endif
		}
		reinterpret_cast<double *>(dst + L.d_scale)[g] = scale;
		reinterpret_cast<double *>(dst + L.d_shift_x)[g] = shift;
		uint32_t *const d_cmd_off = reinterpret_cast<uint32_t *>(dst + L.d_cmd_off);
		d_cmd_off[g] = cmd_at;
		if (g == L.n_glyphs - 1u)
			d_cmd_off[L.n_glyphs] = cmd_at + cmd_n;
		reinterpret_cast<uint16_t *>(dst + L.d_glyph_id)[g] = (uint16_t)gid;
		reinterpret_cast<uint16_t *>(dst + L.d_font_of)[g] = (uint16_t)f;
		if (L.with_pbf) {
			reinterpret_cast<uint32_t *>(dst + L.d_pbf_pre)[g] = pre;
			(dst + L.d_pbf_fix)[g] = (uint8_t)fix;
			names[g] = nm;
		}
		s_cmd_off[t] = cmd_at;
#if FAMILY_PARTS
		uint32_t *const d_part_off = reinterpret_cast<uint32_t *>(dst + L.d_part_off);
		d_part_off[g] = part_at;
		if (g == L.n_glyphs - 1u)
			d_part_off[L.n_glyphs] = part_at + part_n;
		s_part_off[t] = part_at;
		if (t == ng - 1u)
			s_part_off[ng] = part_at + part_n;
		s_gid[t] = (uint16_t)gid;
		s_font[t] = (uint16_t)f;
#endif
#if FAMILY_RECORDS
		if (t == ng - 1u)
			s_cmd_off[ng] = cmd_at + cmd_n;
#endif
	}
	if (__syncthreads_or(bad)) { // (and the barrier in front of the second phase)
		// This workgroup cannot say which parts / records are its own, and the kernels behind it run before the host reads the
		// error word: it overwrites the WHOLE submission's with benign ones — a part without bytes, contours or slots (the
		// decoder reads nothing for it and writes nothing), a close() with no ring open in front of it — racing with the
		// other workgroups' good ones; whichever 16 bytes win, every part names font 0 or its own font and slots inside the
		// batch.  The batch fails in wait either way
#if FAMILY_PARTS
		for (uint32_t j = t; j < n_parts; j += kExpandThreads) {
			uint4 *op = reinterpret_cast<uint4 *>(parts_out + j);
			op[0] = op[1] = op[2] = make_uint4(0, 0, 0, 0);
		}
#endif
#if FAMILY_RECORDS
		for (uint32_t j = t; j < n_cmds; j += kExpandThreads) {
			uint32_t *out = cmds_out + 7ull * j;
			for (uint32_t w = 0; w < 6; w++)
				out[w] = 0;
			out[6] = CMD_CLOSE;
			open_out[j] = 0;
		}
#endif
		return;
	}
#if FAMILY_PARTS && FAMILY_RECORDS
	// both second phases: the leaves of the workgroup's glyf glyphs into parts, then the records of its command glyphs
	{
#include "resident_expand_leaves.inc"
	}
#include "resident_gather_records.inc"
#elif FAMILY_PARTS
#include "resident_expand_leaves.inc"
#else
#include "resident_gather_records.inc"
#endif
}
#undef FAMILY_KERNEL
#undef FAMILY_FONT_REF
#undef FAMILY_PARTS
#undef FAMILY_RECORDS
