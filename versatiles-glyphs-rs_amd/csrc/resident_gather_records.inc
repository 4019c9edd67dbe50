// resident_gather_records.inc — the second phase of the upload kernels that gather command fonts' records and context bytes into
// a submission's command arrays, stamped into resident_gather (glyphs named one by one) and family_gather (code-point ranges of
// families): input_form_kernels.hip.  Expects, in the including kernel: t, ng, n_cmds, cmds_out, open_out, `fonts`, lane t's glyph id
// and font index in gid / f, the LDS arrays s_recs / s_open, and — complete behind a barrier — s_cmd_off[0 .. ng] and s_fonts.
// With RESIDENT_GATHER_MIXED defined (resident_mixed, family_mixed) the list holds fonts of both kinds: a glyph of a glyf font
// leaves no source address, and the slots of such glyphs — they lie inside the workgroup's range, the decoder fills them —
// are passed over.
	if (t < ng) {
		const CommandFontRef ref = f < kExpandFontCache ? s_fonts[f] : fonts[f];
#ifdef RESIDENT_GATHER_MIXED
		if (ref.reserved != kFontRefCommands) {
			s_recs[t] = nullptr;
			s_open[t] = nullptr;
		} else
#endif
		{
			const uint32_t first = reinterpret_cast<const uint32_t *>(ref.cmd_off)[gid];
			s_recs[t] = reinterpret_cast<const uint32_t *>(ref.cmds) + 7ull * first;
			s_open[t] = reinterpret_cast<const uint8_t *>(ref.open) + first;
		}
	}
	__syncthreads();
	const uint32_t c1 = min(s_cmd_off[ng], n_cmds);
	for (uint32_t base = s_cmd_off[0] + t; base < c1; base += kExpandThreads * kGatherUnroll) {
		const uint32_t *rp[kGatherUnroll];
		const uint8_t *op[kGatherUnroll];
#pragma unroll
		for (uint32_t u = 0; u < kGatherUnroll; u++) {
			const uint32_t j = base + u * kExpandThreads;
			// the glyph of command j: the last one whose commands begin at or in front of j (glyphs without commands share an offset)
			uint32_t lo = 0, hi = ng;
			while (hi - lo > 1u) {
				const uint32_t mid = (lo + hi) >> 1;
				if (s_cmd_off[mid] <= j)
					lo = mid;
				else
					hi = mid;
			}
			const uint32_t k = j - s_cmd_off[lo];
#ifdef RESIDENT_GATHER_MIXED
			const uint32_t *const recs = s_recs[lo];
			rp[u] = j < c1 && recs ? recs + 7u * k : nullptr;
			op[u] = rp[u] ? s_open[lo] + k : nullptr;
#else
			rp[u] = j < c1 ? s_recs[lo] + 7u * k : nullptr;
			op[u] = s_open[lo] + k;
#endif
		}
		uint32_t r[kGatherUnroll][7];
		uint8_t o[kGatherUnroll];
#pragma unroll
		for (uint32_t u = 0; u < kGatherUnroll; u++)
			if (rp[u]) {
#pragma unroll
				for (uint32_t w = 0; w < 7; w++)
					r[u][w] = rp[u][w];
				o[u] = *op[u];
			}
#pragma unroll
		for (uint32_t u = 0; u < kGatherUnroll; u++)
			if (rp[u]) {
				const uint32_t j = base + u * kExpandThreads;
				uint32_t *out = cmds_out + 7ull * j;
#pragma unroll
				for (uint32_t w = 0; w < 7; w++)
					out[w] = r[u][w];
				open_out[j] = o[u];
			}
	}
