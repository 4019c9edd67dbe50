// family_table_pass.inc — the text of the family table's passes for workgroup `group` (of kFamilyGroups) of ONE table, included
// as the body of family_tables_pass and of family_tables_batch_pass (family_table_kernels.hip), which name: EMIT, VAR, Var...,
// faces, n_faces, counts (this table's), flags (this table's word), n_entries, table, group, plane and the pack var.  The lanes
// are the 65536 code points of `plane` (0 .. 16); the table keeps their low halves, pbf_fix counts the full value.
	static_assert(VAR ? sizeof...(Var) == 1 || sizeof...(Var) == 2 : sizeof...(Var) == 0, "the variation records come with VAR and only with it");
	__shared__ uint32_t lds_base[kFamilyThreads / 64][3], lds_wave[kFamilyThreads / 64][3];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = (plane << 16) + group * kFamilyThreads + tid;
	const Entry e = find_entry(faces, n_faces, c);
	uint32_t slots = 0, leaves = 0;
	if (e.found) {
		const FamilyFaceRef &F = faces[e.face];
		if (e.gid < F.n_glyph_ids)
			glyph_extent(F, e.gid, slots, leaves);
		else if (!EMIT)
			*flags = FAMILY_FLAG_GLYPH; // (one bit: every writer stores the same word)
	}
	// inclusive sums over the wave, then the earlier waves' totals
	Sum3 inc{e.found ? 1u : 0u, slots, leaves};
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t te = __shfl_up(inc.e, d), ts = __shfl_up(inc.s, d), tl = __shfl_up(inc.l, d);
		if (lane >= d)
			inc.e += te, inc.s += ts, inc.l += tl;
	}
	if (lane == 63)
		lds_wave[wave][0] = inc.e, lds_wave[wave][1] = inc.s, lds_wave[wave][2] = inc.l;
	__syncthreads();
	Sum3 before{0, 0, 0}, total{0, 0, 0};
	for (uint32_t j = 0; j < kFamilyThreads / 64; j++) {
		if (j < wave)
			before.e += lds_wave[j][0], before.s += lds_wave[j][1], before.l += lds_wave[j][2];
		total.e += lds_wave[j][0], total.s += lds_wave[j][1], total.l += lds_wave[j][2];
	}
	if (!EMIT) {
		if (tid == 0) {
			uint32_t *o = counts + kFamilyCounts * group;
			o[0] = total.e, o[1] = total.s, o[2] = total.l, o[3] = 0;
		}
		return;
	}
	// the workgroups in front of this one (tid names a workgroup here: kFamilyGroups == kFamilyThreads)
	static_assert(kFamilyGroups <= kFamilyThreads, "one thread per workgroup's counts");
	Sum3 mine{0, 0, 0};
	if (tid < group)
		mine = Sum3{counts[kFamilyCounts * tid], counts[kFamilyCounts * tid + 1], counts[kFamilyCounts * tid + 2]};
	const Sum3 base = block_sum(mine, lds_base);
	const FamilyTableLayout at(n_entries);
	uint32_t *cmd_pre = (uint32_t *)(table + at.cmd_pre), *leaf_pre = (uint32_t *)(table + at.leaf_pre);
	if (group == kFamilyGroups - 1 && tid == kFamilyThreads - 1 && base.e + total.e == n_entries) {
		cmd_pre[n_entries] = base.s + total.s;
		leaf_pre[n_entries] = base.l + total.l;
	}
	if (!e.found)
		return;
	const uint32_t rank = base.e + before.e + inc.e - 1;
	if (rank >= n_entries) // (never: the host sized the table from the count pass of the same text)
		return;
	const FamilyFaceRef &F = faces[e.face];
	// Face::glyph_hor_advance(gid).value_or(0)
	uint32_t adv = 0;
	if (F.hmtx_len != 0 && F.num_hmetrics != 0 && F.num_glyphs != 0 && e.gid < F.num_glyphs && (uint32_t)F.num_hmetrics * 4u <= F.hmtx_len) {
		const uint32_t i = e.gid < (uint32_t)F.num_hmetrics - 1u ? e.gid : (uint32_t)F.num_hmetrics - 1u;
		adv = be16((const uint8_t *)(uintptr_t)F.hmtx + (size_t)i * 4);
		if constexpr (VAR) { // Face::glyph_hor_advance of a face at a position: f32, `+ 0.5`, truncated; outside u16: none
			const FamilyFaceVar &V = first_of(var...)[e.face];
			float delta;
			bool moved = V.hvar != 0 && hvar_delta(V, e.gid, delta);
			if constexpr (sizeof...(Var) == 2) { // G7: a face without HVAR whose record names the phantom pass's output
				const FamilyFaceGvar &G = second_of(var...)[e.face];
				if (V.hvar == 0 && G.delta != 0 && e.gid < G.n_glyph_ids && ((const uint8_t *)(uintptr_t)G.state)[e.gid] != 2u) {
					delta = ((const float *)(uintptr_t)G.delta)[e.gid];
					moved = true;
				}
			}
			if (moved) {
				const float a = (float)adv + (delta + 0.5f);
				adv = a > -1.0f && a < 65536.0f ? (uint32_t)(int32_t)a : 0u;
			}
		}
	}
	// Renderer::record_resident
	const double scale = 24.0 / (double)F.units_per_em;
	const double advance_float = (double)adv * scale * 0.95;
	const uint32_t advance = (uint32_t)round(advance_float);
	((double *)(table + at.scale))[rank] = scale;
	((double *)(table + at.shift_x))[rank] = ((double)advance - advance_float) / 2.0;
	cmd_pre[rank] = base.s + before.s + inc.s - slots;
	leaf_pre[rank] = base.l + before.l + inc.l - leaves;
	((uint32_t *)(table + at.advance))[rank] = advance;
	((uint16_t *)(table + at.code_point))[rank] = (uint16_t)c;
	((uint16_t *)(table + at.font_of))[rank] = (uint16_t)e.face;
	((uint16_t *)(table + at.glyph_id))[rank] = (uint16_t)e.gid;
	(table + at.pbf_fix)[rank] = (uint8_t)((1u + varint_len(c)) | ((1u + varint_len(advance)) << 4));
