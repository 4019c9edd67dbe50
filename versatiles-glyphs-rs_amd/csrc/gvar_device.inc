// gvar_device.inc — the device functions of the gvar builder, included inside namespace vgsdf { namespace { by the two units that
// hold its kernels: gvar_kernels.hip (one face at one position; its header comment states what a lane does) and
// gvar_batch_kernels.hip (one face at many positions).  First the readers of loca and glyf, the points of a simple entry and the
// contour emitter (what the tree walk calls), then rules G1 to G5 (accumulate: what the deltas pass calls).
__device__ inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
__device__ inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
__device__ inline int32_t bei16(const uint8_t *p) { return (int16_t)be16(p); }
__device__ inline float f2dot14(const uint8_t *p) { return (float)(int16_t)be16(p) / 16384.0f; }

struct Affine {
	float a, b, c, d, e, f;
};
__device__ inline Affine identity() { return Affine{1.f, 0.f, 0.f, 1.f, 0.f, 0.f}; }
__device__ inline bool is_identity(const Affine &t) { return t.a == 1.f && t.b == 0.f && t.c == 0.f && t.d == 1.f && t.e == 0.f && t.f == 0.f; }
// Affine::then: parent.then(child), products and sums in the written order
__device__ inline Affine then(const Affine &p, const Affine &k)
{
	Affine r;
	r.a = p.a * k.a + p.c * k.b;
	r.b = p.b * k.a + p.d * k.b;
	r.c = p.a * k.c + p.c * k.d;
	r.d = p.b * k.c + p.d * k.d;
	r.e = p.a * k.e + p.c * k.f + p.e;
	r.f = p.b * k.e + p.d * k.f + p.f;
	return r;
}
__device__ inline void map(const Affine &t, float &x, float &y)
{
	const float tx = x, ty = y;
	x = t.a * tx + t.c * ty + t.e;
	y = t.b * tx + t.d * ty + t.f;
}

// Face::glyph_data: the glyph id's range [a, b) of glyf, or false
__device__ inline bool glyph_range(const GvarRef &F, uint32_t gid, uint32_t &a, uint32_t &b)
{
	if (F.glyf_len == 0 || gid == 0xFFFFu || gid + 1 >= F.loca_entries)
		return false;
	if (F.loca_long) {
		a = be32(F.loca + (size_t)gid * 4);
		b = be32(F.loca + (size_t)gid * 4 + 4);
	} else {
		a = be16(F.loca + (size_t)gid * 2) * 2;
		b = be16(F.loca + (size_t)gid * 2 + 2) * 2;
	}
	return a < b && b <= F.glyf_len;
}

// ---- walk_simple: the points of a simple entry's body[0, size), one after the other ------------------------------------
enum : uint32_t { ON_CURVE = 0x01, X_SHORT = 0x02, Y_SHORT = 0x04, REPEAT = 0x08, X_SAME_POS = 0x10, Y_SAME_POS = 0x20 };
enum PointsKind : uint32_t { POINTS_FAIL, POINTS_NOTHING, POINTS_OK };
struct Points {
	const uint8_t *body;
	uint32_t n_contours, n_points;
	uint32_t fp, xp, yp, x_at, y_at, y_end;
	uint32_t fl, run_left, contour, in_contour_left;
	int32_t x, y;
};
__device__ inline PointsKind points_open(Points &P, const uint8_t *body, uint32_t size, uint32_t n_contours)
{
	if (n_contours * 2 > size)
		return POINTS_FAIL;
	const uint32_t last_end = be16(body + (n_contours - 1) * 2);
	if (last_end == 0xFFFFu)
		return POINTS_FAIL;
	P.n_points = last_end + 1;
	if (P.n_points == 1)
		return POINTS_NOTHING; // a lone point yields nothing
	uint32_t cur = n_contours * 2;
	if (size - cur < 2)
		return POINTS_FAIL;
	cur += 2 + be16(body + cur); // instructions
	if (cur > size)
		return POINTS_FAIL;
	const uint32_t flags_at = cur;
	uint32_t xs = 0, ys = 0; // (at most 2 x 65536 each)
	for (uint32_t left = P.n_points; left;) {
		if (cur >= size)
			return POINTS_FAIL;
		const uint32_t fl = body[cur++];
		uint32_t run = 1;
		if (fl & REPEAT) {
			if (cur >= size)
				return POINTS_FAIL;
			run += body[cur++];
		}
		if (run > left)
			return POINTS_FAIL;
		xs += (fl & X_SHORT) ? run : ((fl & X_SAME_POS) ? 0 : 2 * run);
		ys += (fl & Y_SHORT) ? run : ((fl & Y_SAME_POS) ? 0 : 2 * run);
		left -= run;
	}
	if ((uint64_t)cur + xs + ys > size)
		return POINTS_FAIL;
	P.body = body, P.n_contours = n_contours;
	P.x_at = cur, P.y_at = cur + xs, P.y_end = cur + xs + ys;
	P.fp = flags_at, P.xp = P.x_at, P.yp = P.y_at;
	P.fl = 0, P.run_left = 0, P.x = 0, P.y = 0;
	P.contour = 1, P.in_contour_left = be16(body); // EndpointsIter
	return POINTS_OK;
}
__device__ inline void points_next(Points &P, int32_t &x, int32_t &y, bool &on_curve, bool &last)
{
	const uint8_t *body = P.body;
	if (P.in_contour_left == 0) {
		if (P.contour < P.n_contours) {
			const uint32_t end = be16(body + P.contour * 2), prev = be16(body + (P.contour - 1) * 2);
			const uint32_t span = end > prev ? end - prev : 0;
			P.in_contour_left = span ? span - 1u : 0u;
		}
		P.contour++;
		last = true;
	} else {
		P.in_contour_left--;
		last = false;
	}
	if (P.run_left == 0) {
		P.fl = P.fp < P.x_at ? body[P.fp++] : 0;
		if (P.fl & REPEAT)
			P.run_left = P.fp < P.x_at ? body[P.fp++] : 0;
	} else {
		P.run_left--;
	}
	const uint32_t fl = P.fl;
	int32_t dx = 0, dy = 0;
	if (fl & X_SHORT) {
		const int32_t v = P.xp < P.y_at ? body[P.xp++] : 0;
		dx = (fl & X_SAME_POS) ? v : -v;
	} else if (!(fl & X_SAME_POS) && P.xp + 2 <= P.y_at) {
		dx = bei16(body + P.xp);
		P.xp += 2;
	}
	if (fl & Y_SHORT) {
		const int32_t v = P.yp < P.y_end ? body[P.yp++] : 0;
		dy = (fl & Y_SAME_POS) ? v : -v;
	} else if (!(fl & Y_SAME_POS) && P.yp + 2 <= P.y_end) {
		dy = bei16(body + P.yp);
		P.yp += 2;
	}
	P.x = (int16_t)(uint16_t)((uint32_t)P.x + (uint32_t)dx); // wrapping
	P.y = (int16_t)(uint16_t)((uint32_t)P.y + (uint32_t)dy);
	x = P.x, y = P.y, on_curve = (fl & ON_CURVE) != 0;
}

// ---- ContourEmitter: points to move / line / quad / close, counted and (EMIT) stored -----------------------------------
struct Out { // a glyph id's commands so far and, for the emit pass, its ranges of kinds and coords
	uint32_t cmds, floats, cmd_cap, dat_cap;
	uint8_t *kinds;
	float *coords;
	uint32_t *flags;
};
template <bool EMIT> __device__ inline void put(Out &o, uint32_t kind, uint32_t n_floats, float a, float b, float c, float d)
{
	if (EMIT) {
		if (o.cmds < o.cmd_cap && o.floats + n_floats <= o.dat_cap) {
			o.kinds[o.cmds] = (uint8_t)kind;
			if (n_floats >= 2)
				o.coords[o.floats] = a, o.coords[o.floats + 1] = b;
			if (n_floats == 4)
				o.coords[o.floats + 2] = c, o.coords[o.floats + 3] = d;
		} else {
			o.flags[GVAR_FLAG_EMIT] = 1;
		}
	}
	o.cmds++, o.floats += n_floats;
}
struct Contour {
	bool has_start, has_lead, has_pending;
	float sx, sy, lx, ly, px, py;
};
template <bool EMIT> struct Emitter {
	Out &o;
	const Affine &t;
	const bool plain;
	Contour c{false, false, false, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

	__device__ void move(float x, float y)
	{
		if (!plain)
			map(t, x, y);
		put<EMIT>(o, 0, 2, x, y, 0.f, 0.f);
	}
	__device__ void line(float x, float y)
	{
		if (!plain)
			map(t, x, y);
		put<EMIT>(o, 1, 2, x, y, 0.f, 0.f);
	}
	__device__ void quad(float cx, float cy, float x, float y)
	{
		if (!plain) {
			map(t, cx, cy);
			map(t, x, y);
		}
		put<EMIT>(o, 2, 4, cx, cy, x, y);
	}
	// lerp(.., 0.5)
	__device__ static float mid(float a, float b) { return a + 0.5f * (b - a); }

	__device__ void point(float x, float y, bool on_curve, bool last_of_contour)
	{
		if (!c.has_start) {
			if (on_curve) {
				c.has_start = true, c.sx = x, c.sy = y;
				move(x, y);
			} else if (c.has_lead) {
				const float mx = mid(c.lx, x), my = mid(c.ly, y);
				c.has_start = true, c.sx = mx, c.sy = my;
				c.has_pending = true, c.px = x, c.py = y;
				move(mx, my);
			} else {
				c.has_lead = true, c.lx = x, c.ly = y;
			}
		} else if (c.has_pending) {
			const float qx = c.px, qy = c.py;
			if (on_curve) {
				c.has_pending = false;
				quad(qx, qy, x, y);
			} else {
				c.px = x, c.py = y;
				quad(qx, qy, mid(qx, x), mid(qy, y));
			}
		} else if (on_curve) {
			line(x, y);
		} else {
			c.has_pending = true, c.px = x, c.py = y;
		}
		if (last_of_contour)
			finish();
	}
	__device__ void finish()
	{
		if (c.has_lead && c.has_pending) {
			const float qx = c.px, qy = c.py;
			c.has_pending = false;
			quad(qx, qy, mid(qx, c.lx), mid(qy, c.ly));
		}
		if (c.has_start && c.has_lead)
			quad(c.lx, c.ly, c.sx, c.sy);
		else if (c.has_start && c.has_pending)
			quad(c.px, c.py, c.sx, c.sy);
		else if (c.has_start)
			line(c.sx, c.sy);
		c.has_start = c.has_lead = c.has_pending = false;
		put<EMIT>(o, 4, 0, 0.f, 0.f, 0.f, 0.f);
	}
};

// a simple entry glyf[pa, pb) (pb - pa >= 10) under transform T; acc (EMIT): the sums of the entry's glyph id, 2 per point.
// false: the entry is malformed (nothing of it was delivered).  n_points: 1 for an entry that yields nothing
template <bool EMIT>
__device__ inline bool leaf(const GvarRef &F, Out &o, uint32_t pa, uint32_t pb, uint32_t n_contours, const Affine &T, const float *acc,
                            uint32_t acc_points, uint32_t &n_points)
{
	Points P;
	const PointsKind kind = points_open(P, F.glyf + pa + 10, pb - pa - 10, n_contours);
	if (kind == POINTS_FAIL)
		return false;
	n_points = P.n_points;
	if (kind == POINTS_NOTHING)
		return true;
	Emitter<EMIT> em{o, T, is_identity(T)};
	for (uint32_t i = 0; i < P.n_points; i++) {
		int32_t x, y;
		bool on_curve, last;
		points_next(P, x, y, on_curve, last);
		float fx = (float)x, fy = (float)y;
		if (EMIT && i < acc_points) // (always: the count pass sized acc by this very entry)
			fx += acc[2 * (size_t)i], fy += acc[2 * (size_t)i + 1];
		em.point(fx, fy, on_curve, last);
	}
	return true;
}

// ---- GvarTable::accumulate: rules G1 to G5 for one glyph id's own entry -----------------------------------------------------
__device__ inline bool has(uint32_t size, uint64_t at, uint64_t n) { return at <= size && n <= size - at; }

// axis_factor (host/cff.cpp)
__device__ inline float axis_factor(int32_t coord, int32_t start, int32_t peak, int32_t end)
{
	if (start > peak || peak > end)
		return 1.0f;
	if (start < 0 && end > 0 && peak != 0)
		return 1.0f;
	if (peak == 0 || coord == peak)
		return 1.0f;
	if (coord <= start || coord >= end)
		return 0.0f;
	if (coord < peak)
		return (float)(coord - start) / (float)(peak - start);
	return (float)(end - coord) / (float)(end - peak);
}

// G2: packed point numbers of b[0, size) from p on, one after the other
struct PointNumbers {
	uint32_t p, count, got, run_left, number;
	bool words, all;
};
__device__ inline bool numbers_open(PointNumbers &N, const uint8_t *b, uint32_t size, uint32_t p)
{
	N.all = false, N.got = 0, N.run_left = 0, N.number = 0, N.words = false, N.count = 0;
	if (p >= size)
		return false;
	uint32_t count = b[p++];
	if (count == 0) {
		N.all = true;
	} else if (count & 0x80u) {
		if (p >= size)
			return false;
		count = ((count & 0x7Fu) << 8) | b[p++];
	}
	N.count = count, N.p = p;
	return true;
}
__device__ inline bool numbers_next(PointNumbers &N, const uint8_t *b, uint32_t size, uint32_t &number)
{
	if (N.run_left == 0) {
		if (N.p >= size)
			return false;
		const uint32_t control = b[N.p++];
		N.words = (control & 0x80u) != 0;
		N.run_left = (control & 0x7Fu) + 1;
	}
	const uint32_t width = N.words ? 2u : 1u;
	if (!has(size, N.p, width))
		return false;
	const uint32_t step = N.words ? be16(b + N.p) : b[N.p];
	N.p += width;
	const uint32_t next = (N.number + step) & 0xFFFFu; // summed in u16
	if (N.got && next <= N.number)
		return false;
	N.number = number = next;
	N.got++, N.run_left--;
	return true;
}
// the numbers from p on are well formed; end: the first byte behind them
__device__ inline bool numbers_check(const uint8_t *b, uint32_t size, uint32_t p, bool &all, uint32_t &end)
{
	PointNumbers N;
	if (!numbers_open(N, b, size, p))
		return false;
	uint32_t number;
	while (N.got < N.count)
		if (!numbers_next(N, b, size, number))
			return false;
	all = N.all, end = N.p;
	return true;
}

// G3: the packed deltas of a tuple as one stream of values
struct DeltaStream {
	const uint8_t *b;
	uint32_t size, p, left, control;
	__device__ bool next(int32_t &v)
	{
		if (left == 0) {
			if (p >= size)
				return false;
			control = b[p++];
			left = (control & 0x3Fu) + 1;
		}
		left--;
		if (control & 0x80u) {
			v = 0;
		} else if (control & 0x40u) {
			if (!has(size, p, 2))
				return false;
			v = bei16(b + p), p += 2;
		} else {
			if (p >= size)
				return false;
			v = (int8_t)b[p], p += 1;
		}
		return true;
	}
};

// G5: what a point at p takes from the touched points at pa (before it) and pb (behind it) of its contour
__device__ inline float inferred(int32_t p, int32_t pa, int32_t pb, float da, float db)
{
	if (pa == pb)
		return da == db ? da : 0.0f;
	if (p <= min(pa, pb))
		return pa < pb ? da : db;
	if (p >= max(pa, pb))
		return pa > pb ? da : db;
	const float d = (float)(p - pa) / (float)(pb - pa);
	return (1.0f - d) * da + d * db;
}

enum : uint32_t { MARK_TOUCHED = 1, MARK_INFERRED = 2, MARK_LAST = 0x80 };
enum DeltasResult : uint32_t { DELTAS_OK, DELTAS_MALFORMED, DELTAS_BUDGET };

// acc[2 * n_all], zeroed; n: the entry's points without the phantom ones; simple: x / y / mark hold the entry's points
__device__ inline DeltasResult accumulate(const GvarRef &F, uint32_t gid, uint32_t n, bool simple, float *acc, float *sx, float *sy,
                                          const int16_t *x, const int16_t *y, uint8_t *mark)
{
	const uint32_t n_all = n + 4;
	const uint8_t *table = F.gvar;
	if (gid >= F.glyph_count)
		return DELTAS_OK;
	// G1
	uint64_t from, to;
	if (F.long_offsets)
		from = be32(table + 20 + (size_t)gid * 4), to = be32(table + 24 + (size_t)gid * 4);
	else
		from = (uint64_t)be16(table + 20 + (size_t)gid * 2) * 2, to = (uint64_t)be16(table + 22 + (size_t)gid * 2) * 2;
	if (from == to)
		return DELTAS_OK;
	if (from > to || !has(F.gvar_len, F.data_at, to))
		return DELTAS_MALFORMED;
	const uint8_t *d = table + F.data_at + from;
	const uint32_t size = (uint32_t)(to - from);
	if (size < 4)
		return DELTAS_MALFORMED;
	const uint32_t n_tuples = be16(d) & 0x0FFFu;
	const bool have_shared = (be16(d) & 0x8000u) != 0;
	if (n_tuples == 0)
		return DELTAS_OK;
	if ((uint64_t)n_tuples * n_all > VGSDF_GVAR_MAX_DELTAS)
		return DELTAS_BUDGET;
	uint32_t cursor = be16(d + 2);
	if (cursor > size)
		return DELTAS_MALFORMED;
	bool shared_all = true;
	uint32_t shared_at = 0;
	if (have_shared) {
		shared_at = cursor;
		if (!numbers_check(d, size, shared_at, shared_all, cursor))
			return DELTAS_MALFORMED;
	}
	uint32_t h = 4;
	const uint32_t tuple_bytes = F.n_axes * 2;
	for (uint32_t t = 0; t < n_tuples; t++) {
		if (!has(size, h, 4))
			return DELTAS_MALFORMED;
		const uint32_t data_size = be16(d + h), index = be16(d + h + 2);
		h += 4;
		const uint8_t *peak, *start = nullptr, *end = nullptr;
		if (index & 0x8000u) {
			if (!has(size, h, tuple_bytes))
				return DELTAS_MALFORMED;
			peak = d + h;
			h += tuple_bytes;
		} else {
			if ((index & 0x0FFFu) >= F.shared_count)
				return DELTAS_MALFORMED;
			peak = table + F.shared_at + (size_t)(index & 0x0FFFu) * tuple_bytes;
		}
		if (index & 0x4000u) {
			if (!has(size, h, 2 * (uint64_t)tuple_bytes))
				return DELTAS_MALFORMED;
			start = d + h, end = d + h + tuple_bytes;
			h += 2 * tuple_bytes;
		}
		if (!has(size, cursor, data_size))
			return DELTAS_MALFORMED;
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
				return DELTAS_MALFORMED;
		}
		DeltaStream deltas{data, data_size, deltas_at, 0, 0};
		int32_t v;
		if (all) {
			for (uint32_t axis = 0; axis < 2; axis++)
				for (uint32_t i = 0; i < n_all; i++) {
					if (!deltas.next(v))
						return DELTAS_MALFORMED;
					acc[2 * (size_t)i + axis] += (float)v * scalar;
				}
			continue;
		}
		for (uint32_t i = 0; i < n_all; i++)
			sx[i] = 0.0f, sy[i] = 0.0f, mark[i] &= MARK_LAST;
		for (uint32_t axis = 0; axis < 2; axis++) {
			PointNumbers N;
			(void)numbers_open(N, nb, nb_size, numbers_at); // (checked above)
			while (N.got < N.count) {
				uint32_t number = 0;
				if (!numbers_next(N, nb, nb_size, number))
					return DELTAS_MALFORMED; // (never: checked above)
				if (!deltas.next(v))
					return DELTAS_MALFORMED;
				if (number < n_all) // (a number at or past the count names no point)
					(axis ? sy : sx)[number] = (float)v * scalar, mark[number] |= MARK_TOUCHED;
			}
		}
		if (simple) {
			for (uint32_t first = 0; first < n;) {
				uint32_t last = first;
				while (last + 1 < n && !(mark[last] & MARK_LAST))
					last++;
				uint32_t lo = 0xFFFFFFFFu, hi = 0;
				for (uint32_t i = first; i <= last; i++)
					if (mark[i] & MARK_TOUCHED)
						lo = min(lo, i), hi = i;
				if (lo != 0xFFFFFFFFu) {
					// (cyclic: in front of the first touched point lies the last one, behind the last the first)
					uint32_t a = hi;
					for (uint32_t i = first; i <= last;) {
						if (mark[i] & MARK_TOUCHED) {
							a = i++;
							continue;
						}
						uint32_t j = i;
						while (j <= last && !(mark[j] & MARK_TOUCHED))
							j++;
						const uint32_t b = j <= last ? j : lo;
						for (; i < j; i++) {
							sx[i] = inferred(x[i], x[a], x[b], sx[a], sx[b]);
							sy[i] = inferred(y[i], y[a], y[b], sy[a], sy[b]);
							mark[i] |= MARK_INFERRED;
						}
					}
				}
				first = last + 1;
			}
		}
		for (uint32_t i = 0; i < n_all; i++)
			if (mark[i] & (MARK_TOUCHED | MARK_INFERRED))
				acc[2 * (size_t)i] += sx[i], acc[2 * (size_t)i + 1] += sy[i];
	}
	return DELTAS_OK;
}

