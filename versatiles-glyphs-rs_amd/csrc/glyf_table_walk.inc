// glyf_table_walk.inc — the walk of one workgroup (one wave) over 64 glyph ids of ONE face, the body of both kernels of
// glyf_table_kernels.hip (the single-face pass and the pass over a batch's faces): one text, so that what a lane does for its
// glyph id cannot differ between them.  The kernel that includes it names, for the workgroup's face: F (GlyfTablesRef), lane, gid
// (the glyph id INSIDE the face), the LDS `stack`, and the face's own counts, leaf_off, byte_at, leaves, bytes and flags.
// Templated on EMIT.
	const bool live = gid < F.n_glyph_ids;
	uint32_t n_leaves = 0, slots = 0, records = 0;
	uint32_t own_len = 0, own_cap = 0, own_body = 0, own_ends = 0, own_cur = 0; // the glyph id's own simple entry
	uint32_t leaf_at = 0, leaf_end = 0;
	if (EMIT && live)
		leaf_at = leaf_off[gid], leaf_end = leaf_off[gid + 1];

	// the composite being read: its depth (-1: none), where its next record is, where its entry ends, its transform
	int depth = -1;
	uint32_t p = 0, end = 0;
	Affine T = identity();
	// a glyph that has been named and resolved, to be entered at depth + 1
	bool pending = false;
	uint32_t pa = 0, pb = 0, pgid = gid;
	Affine PT = identity();
	if (live)
		pending = glyph_range(F, gid, pa, pb);
	bool run = pending;
	while (run) {
		if (pending) { // GlyfWalker::walk(glyph, depth + 1, PT) up to its loop
			pending = false;
			const int d = depth + 1;
			const uint32_t len = pb - pa;
			if (d >= vg::kGlyfMaxComponentDepth || len < 2)
				break; // fails: the whole glyph stops, the leaves so far stay
			const int n_contours = (int16_t)be16(F.glyf + pa);
			if (n_contours > 0) {
				if (len < 10)
					break;
				const Shape sh = measure(F.glyf + pa + 10, len - 10, (uint32_t)n_contours);
				if (sh.kind == SHAPE_FAIL)
					break;
				if (sh.kind == SHAPE_PART) { // ResidentSink::part
					const uint32_t cap = sh.n_points + 2u * (uint32_t)n_contours, byte_len = sh.ends + sh.arrays;
					if ((uint64_t)slots + cap > vg::kResidentMaxGlyphSlots) {
						if (!EMIT)
							flags[GLYF_FLAG_SLOTS] = 1;
						break;
					}
					if (EMIT) {
						const uint32_t at = leaf_at + n_leaves;
						if (at < leaf_end) {
							uint4 *o = (uint4 *)(leaves + (size_t)at * 12);
							o[0] = make_uint4(byte_at[pgid], byte_len, slots, cap);
							o[1] = make_uint4((uint32_t)n_contours, is_identity(PT) ? 1u : 0u, __float_as_uint(PT.a), __float_as_uint(PT.b));
							o[2] = make_uint4(__float_as_uint(PT.c), __float_as_uint(PT.d), __float_as_uint(PT.e), __float_as_uint(PT.f));
						} else {
							flags[GLYF_FLAG_EMIT] = 1;
						}
					}
					if (d == 0)
						own_len = byte_len, own_cap = cap, own_body = pa + 10, own_ends = sh.ends, own_cur = sh.cur;
					slots += cap;
					n_leaves++;
				}
			} else if (n_contours < 0) {
				if (len < 10)
					break;
				if (depth >= 0) { // the composite being read waits on the stack
					uint32_t(*fr)[kGlyfTableLanes] = stack[depth];
					fr[0][lane] = p, fr[1][lane] = end;
					fr[2][lane] = __float_as_uint(T.a), fr[3][lane] = __float_as_uint(T.b), fr[4][lane] = __float_as_uint(T.c);
					fr[5][lane] = __float_as_uint(T.d), fr[6][lane] = __float_as_uint(T.e), fr[7][lane] = __float_as_uint(T.f);
				}
				depth = d, p = pa + 10, end = pb, T = PT;
			}
			if (depth < 0)
				break; // the glyph id itself was simple or empty
			continue;
		}
		// the loop of GlyfWalker::walk over the component records of [p, end); p <= end throughout
		bool more = end - p >= 4;
		if (more) {
			const uint32_t fl = be16(F.glyf + p), child = be16(F.glyf + p + 2);
			p += 4;
			if (++records > VGSDF_GLYF_MAX_COMPONENTS) {
				if (!EMIT)
					flags[GLYF_FLAG_BUDGET] = 1;
				break;
			}
			Affine k = identity();
			if (fl & 0x0002u) { // ARGS_ARE_XY_VALUES (anchor-point arguments are not consumed)
				if (fl & 0x0001u) {
					if ((more = end - p >= 4)) {
						k.e = (float)(int16_t)be16(F.glyf + p);
						k.f = (float)(int16_t)be16(F.glyf + p + 2);
						p += 4;
					}
				} else if ((more = end - p >= 2)) {
					k.e = (float)(int8_t)F.glyf[p];
					k.f = (float)(int8_t)F.glyf[p + 1];
					p += 2;
				}
			}
			if (more) {
				if (fl & 0x0080u) {
					if ((more = end - p >= 8)) {
						k.a = f2dot14(F.glyf + p), k.b = f2dot14(F.glyf + p + 2), k.c = f2dot14(F.glyf + p + 4), k.d = f2dot14(F.glyf + p + 6);
						p += 8;
					}
				} else if (fl & 0x0040u) {
					if ((more = end - p >= 4)) {
						k.a = f2dot14(F.glyf + p), k.d = f2dot14(F.glyf + p + 2);
						p += 4;
					}
				} else if (fl & 0x0008u) {
					if ((more = end - p >= 2)) {
						k.a = k.d = f2dot14(F.glyf + p);
						p += 2;
					}
				}
			}
			if (more) {
				if (!(fl & 0x0020u)) // no MORE_COMPONENTS: the loop ends behind this child
					p = end;
				if (glyph_range(F, child, pa, pb)) {
					pending = true;
					pgid = child;
					PT = then(T, k);
				}
				continue;
			}
		}
		// the records are through (or one was truncated): walk returns true, its caller goes on
		depth--;
		if (depth < 0)
			break;
		const uint32_t(*fr)[kGlyfTableLanes] = stack[depth];
		p = fr[0][lane], end = fr[1][lane];
		T.a = __uint_as_float(fr[2][lane]), T.b = __uint_as_float(fr[3][lane]), T.c = __uint_as_float(fr[4][lane]);
		T.d = __uint_as_float(fr[5][lane]), T.e = __uint_as_float(fr[6][lane]), T.f = __uint_as_float(fr[7][lane]);
	}

	if (!EMIT) {
		if (live)
			((uint4 *)counts)[gid] = make_uint4(own_len, n_leaves, slots, own_cap);
		return;
	}
	// the simple entries' bytes, the whole wave over one entry after the other: endPtsOfContours, then what lies behind the
	// instructions, zero-padded to the next multiple of 4.  The source has any alignment: bytes in, words out
	uint32_t dst = 0, dst_end = 0;
	if (own_len)
		dst = byte_at[gid], dst_end = byte_at[gid + 1];
	for (unsigned long long m = __ballot(own_len != 0); m; m &= m - 1) {
		const int j = __ffsll(m) - 1;
		const uint32_t body = __shfl(own_body, j), ends = __shfl(own_ends, j), cur = __shfl(own_cur, j), len = __shfl(own_len, j);
		const uint32_t to = __shfl(dst, j), to_end = __shfl(dst_end, j);
		const uint8_t *src = F.glyf + body;
		for (uint32_t w = lane; w < (len + 3) / 4; w += kGlyfTableLanes) {
			uint32_t word = 0;
			for (uint32_t i = 0; i < 4; i++) {
				const uint32_t at = 4 * w + i;
				if (at < len)
					word |= (uint32_t)(at < ends ? src[at] : src[cur + (at - ends)]) << (8 * i);
			}
			if (4 * w + 4 <= to_end - to)
				*(uint32_t *)(bytes + to + 4 * (size_t)w) = word;
			else
				flags[GLYF_FLAG_EMIT] = 1;
		}
	}
