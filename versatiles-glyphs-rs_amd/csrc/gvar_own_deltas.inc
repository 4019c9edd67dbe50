// gvar_own_deltas.inc — the deltas pass's share of one lane's glyph id, the body of gvar_deltas_pass (gvar_kernels.hip) and of
// gvar_batch_deltas_pass (gvar_batch_kernels.hip): one text.  The kernel that includes it names: F (GvarRef, coords those of the
// lane's position), gid, g0 (the first glyph id of the launch), counts, pt_at, acc_all and flags (the position's) and S, the
// scratch of the launch's glyph ids at the lane's position.
	const uint32_t n_all = counts[(size_t)kGvarCounts * gid];
	uint32_t pa = 0, pb = 0;
	if (n_all < 4 || !glyph_range(F, gid, pa, pb) || pb - pa < 10)
		return;
	const uint32_t n = n_all - 4, base = pt_at[gid], at = base - pt_at[g0];
	float *acc = acc_all + 2 * (size_t)base;
	for (uint32_t i = 0; i < 2 * n_all; i++)
		acc[i] = 0.0f;
	float *sx = S.sx + at, *sy = S.sy + at;
	int16_t *x = S.x + at, *y = S.y + at;
	uint8_t *mark = S.mark + at;
	const int n_contours = (int16_t)be16(F.glyf + pa);
	const bool simple = n_contours > 0;
	for (uint32_t i = 0; i < n_all; i++)
		mark[i] = 0;
	if (simple) {
		Points P;
		if (points_open(P, F.glyf + pa + 10, pb - pa - 10, (uint32_t)n_contours) != POINTS_OK || P.n_points != n)
			return; // (never: the count pass opened this very entry)
		for (uint32_t i = 0; i < n; i++) {
			int32_t px, py;
			bool on_curve, last;
			points_next(P, px, py, on_curve, last);
			x[i] = (int16_t)px, y[i] = (int16_t)py, mark[i] = last ? MARK_LAST : 0;
		}
	}
	const DeltasResult r = accumulate(F, gid, n, simple, acc, sx, sy, x, y, mark);
	if (r == DELTAS_MALFORMED)
		flags[GVAR_FLAG_MALFORMED] = 1;
	else if (r == DELTAS_BUDGET)
		flags[GVAR_FLAG_DELTAS] = 1;
