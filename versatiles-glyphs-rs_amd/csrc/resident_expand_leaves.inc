// resident_expand_leaves.inc — the second phase of the upload kernels that expand resident `glyf` fonts' leaves into a
// submission's parts, stamped into resident_expand (glyphs named one by one) and family_expand (code-point ranges of families):
// input_form_kernels.hip.  Expects, in the including kernel: t (threadIdx.x), ng (glyphs of this workgroup), n_parts, parts_out,
// `fonts` (the block's font references) and, in LDS and complete behind a barrier, s_part_off[0 .. ng], s_cmd_off, s_gid, s_font
// [0 .. ng) and s_fonts (the first kExpandFontCache references).
	const uint32_t p1 = min(s_part_off[ng], n_parts);
	for (uint32_t j = s_part_off[0] + t; j < p1; j += kExpandThreads) {
		// the glyph of part j: the last one whose parts begin at or in front of j (glyphs without leaves share an offset)
		uint32_t lo = 0, hi = ng;
		while (hi - lo > 1u) {
			const uint32_t mid = (lo + hi) >> 1;
			if (s_part_off[mid] <= j)
				lo = mid;
			else
				hi = mid;
		}
		const uint32_t f = s_font[lo];
		const ResidentFontRef ref = f < kExpandFontCache ? s_fonts[f] : fonts[f];
		const uint32_t leaf = reinterpret_cast<const uint32_t *>(ref.leaf_off)[s_gid[lo]] + (j - s_part_off[lo]);
		const uint4 *lp = reinterpret_cast<const uint4 *>(reinterpret_cast<const GlyfPart *>(ref.leaves) + leaf);
		uint4 r0 = lp[0], r1 = lp[1];
		const uint4 r2 = lp[2];
		r0.z += s_cmd_off[lo]; // cmd_at: from the glyph's first slot -> in the batch
		r1.y |= f << 16;       // plain | font index (glyf_decode_resident)
		uint4 *op = reinterpret_cast<uint4 *>(parts_out + j);
		op[0] = r0;
		op[1] = r1;
		op[2] = r2;
	}
