// gvar_tree_walk.inc — GvarWalker::walk for one lane's glyph id, the body of the count and emit kernels of gvar_kernels.hip and
// of the emit kernel of gvar_batch_kernels.hip: one text, so that what a lane does for its glyph id cannot differ between them.
// The kernel that includes it names: F (GvarRef), lane, gid, the LDS `stack`, counts, pt_at and, for the store the lane writes to,
// acc, cmd_off, dat_off, kinds, coords and flags.  Templated on EMIT.
	const bool live = gid < F.n_glyph_ids;
	Out o{0, 0, 0, 0, nullptr, nullptr, flags};
	if (EMIT && live) {
		const uint32_t c0 = cmd_off[gid], c1 = cmd_off[gid + 1], d0 = dat_off[gid], d1 = dat_off[gid + 1];
		o.cmd_cap = c1 - c0, o.dat_cap = d1 - d0, o.kinds = kinds + c0, o.coords = coords + d0;
	}
	uint32_t own_points = 0, records = 0;

	// the composite being read: its depth (-1: none), its glyph id, where its next record is and which it is, where its entry
	// ends, its transform
	int depth = -1;
	uint32_t p = 0, end = 0, cur = 0, rec = 0;
	Affine T = identity();
	// a glyph that has been named and resolved, to be entered at depth + 1
	bool pending = false;
	uint32_t pa = 0, pb = 0, pgid = gid;
	Affine PT = identity();
	if (live)
		pending = glyph_range(F, gid, pa, pb);
	bool run = pending;
	while (run) {
		if (pending) { // GvarWalker::walk(pgid, depth + 1, PT) up to its second loop
			pending = false;
			const int d = depth + 1;
			const uint32_t len = pb - pa;
			if (d >= vg::kGlyfMaxComponentDepth || len < 2)
				break; // fails: the whole glyph stops, the commands so far stay
			const int n_contours = (int16_t)be16(F.glyf + pa);
			if (n_contours > 0) {
				if (len < 10)
					break;
				uint32_t n_points = 1, acc_points = 0;
				const float *sums = nullptr;
				if (EMIT) {
					const uint32_t own = counts[(size_t)kGvarCounts * pgid];
					acc_points = own ? own - 4 : 0;
					sums = acc + 2 * (size_t)pt_at[pgid];
				}
				if (!leaf<EMIT>(F, o, pa, pb, (uint32_t)n_contours, PT, sums, acc_points, n_points))
					break;
				if (d == 0 && n_points > 1)
					own_points = n_points + 4;
				if (o.cmds > vg::kGvarMaxGlyphCmds) {
					if (!EMIT)
						flags[GVAR_FLAG_CMDS] = 1;
					break;
				}
			} else if (n_contours < 0) {
				if (len < 10)
					break;
				if (d == 0) { // the entry's own points: one per record that is read whole
					uint32_t n = 0;
					for (uint32_t q = pa + 10; pb - q >= 4;) {
						const uint32_t fl = be16(F.glyf + q);
						const uint32_t args = (fl & 0x0002u) ? ((fl & 0x0001u) ? 4u : 2u) : 0u;
						const uint32_t scale = (fl & 0x0080u) ? 8u : ((fl & 0x0040u) ? 4u : ((fl & 0x0008u) ? 2u : 0u));
						// (read_component checks the arguments, then the scale: together they fail alike)
						if (pb - q - 4 < args + scale)
							break;
						q += 4 + args + scale;
						n++;
						if (!(fl & 0x0020u) || n > vg::kGvarMaxRecords)
							break;
					}
					if (n > vg::kGvarMaxRecords) {
						if (!EMIT)
							flags[GVAR_FLAG_RECORDS] = 1;
						break;
					}
					own_points = n + 4;
				}
				if (depth >= 0) { // the composite being read waits on the stack
					uint32_t(*fr)[kGvarLanes] = stack[depth];
					fr[0][lane] = p, fr[1][lane] = cur | (rec << 16);
					fr[2][lane] = __float_as_uint(T.a), fr[3][lane] = __float_as_uint(T.b), fr[4][lane] = __float_as_uint(T.c);
					fr[5][lane] = __float_as_uint(T.d), fr[6][lane] = __float_as_uint(T.e), fr[7][lane] = __float_as_uint(T.f);
				}
				depth = d, p = pa + 10, end = pb, T = PT, cur = pgid, rec = 0;
			}
			if (depth < 0)
				break; // the glyph id itself was simple or empty
			continue;
		}
		// the loop of GvarWalker::walk over the component records of [p, end); p <= end throughout
		bool more = end - p >= 4;
		if (more) {
			const uint32_t fl = be16(F.glyf + p), child = be16(F.glyf + p + 2);
			p += 4;
			if (++records > VGSDF_GLYF_MAX_COMPONENTS) {
				if (!EMIT)
					flags[GVAR_FLAG_RECORDS] = 1;
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
				if (EMIT) { // G6: the record's offsets take the composite's sums before the transforms are combined
					const uint32_t own = counts[(size_t)kGvarCounts * cur];
					if (own >= 4 && rec < own - 4) { // (always: the count pass sized acc by this very entry)
						const float *sums = acc + 2 * ((size_t)pt_at[cur] + rec);
						k.e += sums[0], k.f += sums[1];
					}
				}
				rec = (rec + 1) & 0xFFFFu; // (a composite of more records has been refused by the count pass of its own glyph id)
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
		const uint32_t(*fr)[kGvarLanes] = stack[depth];
		p = fr[0][lane], cur = fr[1][lane] & 0xFFFFu, rec = fr[1][lane] >> 16;
		T.a = __uint_as_float(fr[2][lane]), T.b = __uint_as_float(fr[3][lane]), T.c = __uint_as_float(fr[4][lane]);
		T.d = __uint_as_float(fr[5][lane]), T.e = __uint_as_float(fr[6][lane]), T.f = __uint_as_float(fr[7][lane]);
		// (a composite on the stack resolved when it was entered: glyph_range answers as it did then; were it not so, no record more)
		uint32_t from = 0, to = 0;
		end = glyph_range(F, cur, from, to) && to >= p ? to : p;
	}

	if (EMIT) {
		if (live && (o.cmds != o.cmd_cap || o.floats != o.dat_cap))
			flags[GVAR_FLAG_EMIT] = 1;
		return;
	}
	if (live)
		((uint4 *)counts)[gid] = make_uint4(own_points, o.cmds, o.floats, 0);
