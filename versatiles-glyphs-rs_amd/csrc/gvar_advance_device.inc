// gvar_advance_device.inc — what a lane of the phantom pass does for a glyph id, included inside namespace vgsdf's anonymous
// namespace behind gvar_device.inc by gvar_advance_kernels.hip (one lane per glyph id) and gvar_advance_batch_kernels.hip (one lane
// per (glyph id, position) pair): Face::own_point_count, then GvarTable::phantom_sums over F.coords.

// Face::own_point_count: the points of the glyph id's own entry; false: the entry is malformed
__device__ inline bool own_point_count(const GvarRef &F, uint32_t gid, uint32_t &n)
{
	n = 0;
	uint32_t a, b;
	if (!glyph_range(F, gid, a, b))
		return true; // no entry: no point, and still the four phantom ones
	const uint32_t size = b - a;
	if (size < 2)
		return false;
	const int32_t n_contours = bei16(F.glyf + a);
	if (n_contours == 0)
		return true;
	if (size < 10)
		return false;
	const uint8_t *body = F.glyf + a + 10;
	const uint32_t body_size = size - 10;
	if (n_contours > 0) {
		if ((uint32_t)n_contours * 2 > body_size)
			return false;
		const uint32_t last_end = be16(body + ((uint32_t)n_contours - 1) * 2);
		if (last_end == 0xFFFFu)
			return false;
		n = last_end + 1;
		return true;
	}
	for (uint32_t p = 0;;) { // composite: one point per record the static walk reads (read_component's sizes)
		if (!has(body_size, p, 4))
			break;
		const uint32_t flags = be16(body + p);
		p += 4;
		if (flags & 0x0002u) {
			const uint32_t w = (flags & 0x0001u) ? 4u : 2u;
			if (!has(body_size, p, w))
				break;
			p += w;
		}
		const uint32_t t = (flags & 0x0080u) ? 8u : (flags & 0x0040u) ? 4u : (flags & 0x0008u) ? 2u : 0u;
		if (!has(body_size, p, t))
			break;
		p += t;
		n++;
		if (!(flags & 0x0020u))
			break;
	}
	return true;
}

// a scaled x delta of point `number`: l += c for point n, r += c for point n + 1 (both sums formed, one kept: the accumulators
// stay in registers)
__device__ inline void take(float &l, float &r, uint32_t number, uint32_t n, float c)
{
	const float nl = l + c, nr = r + c;
	l = number == n ? nl : l;
	r = number == n + 1 ? nr : r;
}

// GvarTable::phantom_sums
__device__ inline uint32_t phantom_sums(const GvarRef &F, uint32_t gid, uint32_t n, float &l, float &r, uint32_t *flags)
{
	l = r = 0.0f;
	const uint8_t *table = F.gvar;
	if (gid >= F.glyph_count)
		return GVAR_ADVANCE_NONE;
	// G1
	uint64_t from, to;
	if (F.long_offsets)
		from = be32(table + 20 + (size_t)gid * 4), to = be32(table + 24 + (size_t)gid * 4);
	else
		from = (uint64_t)be16(table + 20 + (size_t)gid * 2) * 2, to = (uint64_t)be16(table + 22 + (size_t)gid * 2) * 2;
	if (from == to)
		return GVAR_ADVANCE_NONE;
	if (from > to || !has(F.gvar_len, F.data_at, to))
		return GVAR_ADVANCE_MALFORMED;
	const uint8_t *d = table + F.data_at + from;
	const uint32_t size = (uint32_t)(to - from);
	if (size < 4)
		return GVAR_ADVANCE_MALFORMED;
	const uint32_t n_tuples = be16(d) & 0x0FFFu;
	const bool have_shared = (be16(d) & 0x8000u) != 0;
	if (n_tuples == 0)
		return GVAR_ADVANCE_NONE;
	if ((uint64_t)n_tuples * (n + 4) > VGSDF_GVAR_MAX_DELTAS) {
		flags[GVAR_ADVANCE_FLAG_DELTAS] = 1;
		return GVAR_ADVANCE_MALFORMED; // (the call is refused: nobody reads this)
	}
	uint32_t cursor = be16(d + 2);
	if (cursor > size)
		return GVAR_ADVANCE_MALFORMED;
	bool shared_all = true;
	uint32_t shared_at = 0;
	if (have_shared) {
		shared_at = cursor;
		if (!numbers_check(d, size, shared_at, shared_all, cursor))
			return GVAR_ADVANCE_MALFORMED;
	}
	uint32_t h = 4;
	const uint32_t tuple_bytes = F.n_axes * 2;
	for (uint32_t t = 0; t < n_tuples; t++) {
		if (!has(size, h, 4))
			return GVAR_ADVANCE_MALFORMED;
		const uint32_t data_size = be16(d + h), index = be16(d + h + 2);
		h += 4;
		const uint8_t *peak, *start = nullptr, *end = nullptr;
		if (index & 0x8000u) {
			if (!has(size, h, tuple_bytes))
				return GVAR_ADVANCE_MALFORMED;
			peak = d + h;
			h += tuple_bytes;
		} else {
			if ((index & 0x0FFFu) >= F.shared_count)
				return GVAR_ADVANCE_MALFORMED;
			peak = table + F.shared_at + (size_t)(index & 0x0FFFu) * tuple_bytes;
		}
		if (index & 0x4000u) {
			if (!has(size, h, 2 * (uint64_t)tuple_bytes))
				return GVAR_ADVANCE_MALFORMED;
			start = d + h, end = d + h + tuple_bytes;
			h += 2 * tuple_bytes;
		}
		if (!has(size, cursor, data_size))
			return GVAR_ADVANCE_MALFORMED;
		const uint8_t *data = d + cursor;
		cursor += data_size;
		// G4
		float scalar = 1.0f;
		for (uint32_t i = 0; i < F.n_axes && scalar != 0.0f; i++) {
			const int32_t pk = bei16(peak + 2 * i);
			const int32_t st = start ? bei16(start + 2 * i) : min(pk, 0);
			const int32_t en = end ? bei16(end + 2 * i) : max(pk, 0);
			const float f = axis_factor(F.coords[i], st, pk, en);
			scalar = f == 0.0f ? 0.0f : scalar * f;
		}
		if (scalar == 0.0f)
			continue;
		// the tuple's point numbers: its own (in its data, the deltas behind them) or the shared ones
		const uint8_t *nb = d;
		uint32_t nb_size = size, numbers_at = shared_at, deltas_at = 0;
		bool all = shared_all;
		if (index & 0x2000u) {
			nb = data, nb_size = data_size, numbers_at = 0;
			if (!numbers_check(data, data_size, 0, all, deltas_at))
				return GVAR_ADVANCE_MALFORMED;
		}
		DeltaStream deltas{data, data_size, deltas_at, 0, 0};
		int32_t v;
		if (all) {
			for (uint32_t i = 0; i < 2 * (n + 4); i++) { // the x deltas first
				if (!deltas.next(v))
					return GVAR_ADVANCE_MALFORMED;
				take(l, r, i, n, (float)v * scalar);
			}
			continue;
		}
		PointNumbers N;
		(void)numbers_open(N, nb, nb_size, numbers_at); // (checked above)
		while (N.got < N.count) {
			uint32_t number = 0;
			if (!numbers_next(N, nb, nb_size, number) || !deltas.next(v))
				return GVAR_ADVANCE_MALFORMED;
			take(l, r, number, n, (float)v * scalar);
		}
		for (uint32_t i = 0; i < N.count; i++) // the y deltas
			if (!deltas.next(v))
				return GVAR_ADVANCE_MALFORMED;
	}
	return GVAR_ADVANCE_DELTA;
}
