// outline_union_pass.inc — the body of outline_union_pass<EMIT> (outline_union_kernels.hip): one workgroup per glyph, lanes over
// its segments in rounds of kUnionLanes, the partner loop over the window in LDS.  Rule U (DESIGN.md §7), in the operation
// order tests/union_outline_kit.py restates.  A lane walks its segment from cut to cut: one sweep over the partners finds the
// lowest cut above the one it stands on, a second classifies the piece between the two at its midpoint, so no lane keeps a
// list of cuts.  Every barrier below is reached by all lanes: the conditions around them are workgroup-wide votes.
	__shared__ double wsx[VGSDF_UNION_WINDOW], wsy[VGSDF_UNION_WINDOW], wex[VGSDF_UNION_WINDOW], wey[VGSDF_UNION_WINDOW];
	__shared__ uint32_t part[kUnionLanes];
	const uint32_t g = blockIdx.x, lane = threadIdx.x;
	const GlyphDesc desc = glyphs[g];
	const uint32_t N = desc.n_seg;
	const size_t first = desc.seg_off;
	const auto in = [&](const double *a, uint32_t q) { return a[(first + q) * seg_stride]; };

	uint32_t st;
	if constexpr (EMIT) {
		st = state[g];
	} else {
		st = VGSDF_UNION_IDENTITY;
		if (N > VGSDF_UNION_MAX_SEGMENTS) {
			st = VGSDF_UNION_OVER_LIMIT;
		} else {
			bool bad = false;
			for (uint32_t q = lane; q < N; q += kUnionLanes)
				bad |= !(__builtin_isfinite(in(sx, q)) && __builtin_isfinite(in(sy, q)) && __builtin_isfinite(in(ex, q)) &&
				         __builtin_isfinite(in(ey, q)));
			if (__syncthreads_or(bad))
				st = VGSDF_UNION_NON_FINITE;
		}
	}
	if (st >= VGSDF_UNION_OVER_LIMIT) { // passed through unchanged
		if constexpr (EMIT) {
			const uint32_t lo = piece_off[g], room = piece_off[g + 1] - lo;
			for (uint32_t q = lane; q < N && q < room; q += kUnionLanes) {
				const size_t o = (size_t)(lo + q) * out_stride;
				out_sx[o] = in(sx, q), out_sy[o] = in(sy, q), out_ex[o] = in(ex, q), out_ey[o] = in(ey, q);
			}
		} else if (lane == 0) {
			piece_count[g] = N, state[g] = (uint8_t)st;
		}
		return;
	}

	const auto stage = [&](uint32_t w0) {
		const uint32_t m = min((uint32_t)VGSDF_UNION_WINDOW, N - w0);
		for (uint32_t q = lane; q < m; q += kUnionLanes)
			wsx[q] = in(sx, w0 + q), wsy[q] = in(sy, w0 + q), wex[q] = in(ex, w0 + q), wey[q] = in(ey, w0 + q);
	};
	const bool resident = N <= VGSDF_UNION_WINDOW; // staged once
	if (resident) {
		stage(0);
		__syncthreads();
	}
	// body(p, P) for every partner p < N in index order
	const auto for_partners = [&](auto &&body) {
		for (uint32_t w0 = 0; w0 < N; w0 += VGSDF_UNION_WINDOW) {
			if (!resident) {
				__syncthreads(); // the window's readers are through
				stage(w0);
				__syncthreads();
			}
			const uint32_t m = min((uint32_t)VGSDF_UNION_WINDOW, N - w0);
			for (uint32_t q = 0; q < m; q++)
				body(w0 + q, Seg{wsx[q], wsy[q], wex[q], wey[q]});
		}
	};

	uint32_t running = 0; // pieces of the rounds before this one
	bool changed = false;
	const uint32_t out_lo = EMIT ? piece_off[g] : 0, out_hi = EMIT ? piece_off[g + 1] : 0;
	for (uint32_t base = 0; base < N; base += kUnionLanes) {
		const uint32_t k = base + lane;
		const bool has = k < N;
		Seg K{0.0, 0.0, 0.0, 0.0};
		if (has)
			K = Seg{in(sx, k), in(sy, k), in(ex, k), in(ey, k)};
		const double dkx = K.ex - K.sx, dky = K.ey - K.sy;
		const bool steep = fabs(dky) >= fabs(dkx);  // the ray of the classification: horizontal, else x and y exchanged
		const int sg = (steep ? dky : dkx) > 0.0 ? 1 : -1;
		bool active = has && !zero_length(K);
		uint32_t n_mine = 0, at = 0;
		if constexpr (EMIT)
			at = has ? out_lo + seg_first[first + k] : 0;
		double cur_t = 0.0, cx = K.sx, cy = K.sy;
		for (uint32_t it = 0; it < 2 * N + 2; it++) { // (a segment has at most 2 (N - 1) cuts)
			if (!__syncthreads_or(active))
				break;
			// the lowest cut above cur_t; among equals the partner of lowest index
			double best_t = 1.0, bx = K.ex, by = K.ey;
			for_partners([&](uint32_t p, const Seg &P) {
				if (active && p != k && !zero_length(P))
					next_cut(K, k, dkx, dky, P, p, cur_t, best_t, bx, by);
			});
			const bool found = best_t < 1.0;
			const bool piece = active && !(cx == bx && cy == by);
			if (__syncthreads_or(piece)) {
				double mx = (cx + bx) * 0.5, my = (cy + by) * 0.5;
				if (!steep) {
					const double m = mx;
					mx = my, my = m;
				}
				int w = 0, step = sg;
				bool lower_same = false;
				for_partners([&](uint32_t p, const Seg &P) {
					if (piece && p != k && !zero_length(P))
						classify(K, k, P, p, steep, mx, my, sg, w, step, lower_same);
				});
				const bool keep = ((w == 0) != (w + step == 0)) && ((step > 0) == (sg > 0)) && !lower_same;
				if (piece && keep) {
					if constexpr (EMIT) {
						if (at + n_mine < out_hi) {
							const size_t o = (size_t)(at + n_mine) * out_stride;
							out_sx[o] = cx, out_sy[o] = cy, out_ex[o] = bx, out_ey[o] = by;
						}
					}
					n_mine++;
				}
				changed |= piece && !keep;
			}
			changed |= active && found;
			if (found)
				cur_t = best_t, cx = bx, cy = by;
			else
				active = false;
		}
		if constexpr (!EMIT) { // the place of each segment's first piece: a running sum in segment order
			part[lane] = n_mine;
			__syncthreads();
			uint32_t before = 0, total = 0;
			for (uint32_t q = 0; q < kUnionLanes; q++) {
				const uint32_t c = part[q];
				before += q < lane ? c : 0;
				total += c;
			}
			if (has)
				seg_first[first + k] = running + before;
			running += total;
			__syncthreads();
		}
	}
	if constexpr (!EMIT) {
		const int any = __syncthreads_or(changed);
		if (lane == 0)
			piece_count[g] = running, state[g] = any ? VGSDF_UNION_REBUILT : VGSDF_UNION_IDENTITY;
	}
