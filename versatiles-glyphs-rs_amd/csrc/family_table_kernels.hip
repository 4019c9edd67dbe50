// family_table_kernels.hip — a font id's table code point -> (font, glyph id, advance, scale, shift_x) from its faces' `cmap` and
// `hmtx` bytes (family_table_kernels.h).  What a lane computes for its code point is, step for step, what the host computes in
// FontManager::family_table: the face is the first in order that MAPS the code point (a unicode subtable lists it and its
// lookup has a value: Face::unicode_codepoints), the glyph id is the first value any of that face's subtables has
// (Face::glyph_index), and the entry's numbers are Renderer::record_resident's in f64 (this unit is built with
// -ffp-contract=off).  The lookups are CmapSubtable::glyph_index's bisections; every read is bounded by the table lengths of the
// face record.  Two passes of one text: the count pass leaves per workgroup its entries, command slots and leaves, the emit pass
// places every entry at its rank and writes all nine arrays of FamilyTableLayout.  A third instantiation of that text, the emit
// pass with VAR, adds to the `hmtx` advance of a face at a position what Face::hvar_advance_delta finds in the face's `HVAR`; a
// fourth, VAR with a second record array, adds for a face without `HVAR` what the phantom pass found in its `gvar` (rule G7).
#include "family_table_kernels.h"

#include "upload_layout.h"

namespace vgsdf {
namespace {

// a cmap subtable: from its first byte to the END OF THE CMAP TABLE (the bound of data.has on the host)
struct Sub {
	const uint8_t *p;
	uint64_t n;
};
__device__ inline bool has(const Sub &d, uint64_t off, uint64_t len) { return off <= d.n && len <= d.n - off; }
__device__ inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
__device__ inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// CmapSubtable::glyph_index: the glyph id, or -1 for "no value"; listed: for_each_codepoint visits c (meaningful with a value)
__device__ int32_t lookup(const Sub &d, uint32_t format, uint32_t c, bool &listed)
{
	listed = true;
	switch (format) {
	case 0: {
		if (c >= 256 || !has(d, 6, 256))
			return -1;
		const uint32_t g = d.p[6 + c];
		return g ? (int32_t)g : -1;
	}
	case 4: {
		if (!has(d, 0, 14))
			return -1;
		const uint32_t x2 = be16(d.p + 6);
		if (x2 < 2)
			return -1;
		const uint32_t segs = x2 / 2, ends = 14, starts = ends + segs * 2 + 2, deltas = starts + segs * 2, offsets = deltas + segs * 2;
		if (!has(d, offsets, segs * 2))
			return -1;
		uint32_t lo = 0, hi = segs;
		while (lo < hi) {
			const uint32_t mid = (lo + hi) / 2;
			const uint32_t end = be16(d.p + ends + mid * 2);
			if (end < c) {
				lo = mid + 1;
				continue;
			}
			const uint32_t first = be16(d.p + starts + mid * 2);
			if (first > c) {
				hi = mid;
				continue;
			}
			listed = !(first == 0xFFFFu && end == 0xFFFFu); // the closing segment is not enumerated
			const uint32_t range_off = be16(d.p + offsets + mid * 2), delta = be16(d.p + deltas + mid * 2);
			if (range_off == 0)
				return (int32_t)((c + delta) & 0xFFFFu);
			if (range_off == 0xFFFFu)
				return -1;
			const uint32_t twice = (c - first) * 2;
			if (twice > 0xFFFFu)
				return -1;
			const uint32_t pos = (offsets + mid * 2 + twice + range_off) & 0xFFFFu; // wraps in u16, from the subtable start
			if (!has(d, pos, 2))
				return -1;
			const uint32_t raw = be16(d.p + pos);
			if (raw == 0)
				return -1;
			const uint32_t id = (raw + delta) & 0xFFFFu;
			return id & 0x8000u ? -1 : (int32_t)id; // negative as i16
		}
		return -1;
	}
	case 6: {
		if (c > 0xFFFFu || !has(d, 0, 10)) // (a 16-bit format: nothing above the BMP, wherever first + count reaches)
			return -1;
		const uint32_t first = be16(d.p + 6), count = be16(d.p + 8);
		if (c < first || c - first >= count || !has(d, 10 + (uint64_t)(c - first) * 2, 2))
			return -1;
		return (int32_t)be16(d.p + 10 + (size_t)(c - first) * 2);
	}
	case 10: {
		if (!has(d, 0, 20))
			return -1;
		const uint32_t first = be32(d.p + 12), count = be32(d.p + 16);
		if (c < first || c - first >= count || !has(d, 20 + (uint64_t)(c - first) * 2, 2))
			return -1;
		return (int32_t)be16(d.p + 20 + (size_t)(c - first) * 2);
	}
	case 12:
	case 13: {
		if (!has(d, 0, 16))
			return -1;
		const uint32_t n = be32(d.p + 12);
		if (!has(d, 16, (uint64_t)n * 12))
			return -1;
		uint32_t lo = 0, hi = n;
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo) / 2;
			const uint8_t *g = d.p + 16 + (size_t)mid * 12;
			const uint32_t start = be32(g);
			if (start > c)
				hi = mid;
			else if (be32(g + 4) < c)
				lo = mid + 1;
			else {
				uint64_t id = be32(g + 8);
				if (format == 12)
					id = id + c - start; // (c <= 0x10FFFF: below 2^33; an id + c past 2^32 - 1, which the reader refuses, has id > 0xFFFF)
				return id > 0xFFFFu ? -1 : (int32_t)id;
			}
		}
		return -1;
	}
	default:
		return -1;
	}
}

struct Entry {
	bool found;
	uint32_t face, gid;
};

__device__ Entry find_entry(const FamilyFaceRef *faces, uint32_t n_faces, uint32_t c)
{
	Entry e{false, 0, 0};
	if (c >= 0xD800u && c <= 0xDFFFu)
		return e;
	for (uint32_t k = 0; k < n_faces; k++) {
		const FamilyFaceRef &F = faces[k];
		const FamilySubtable *subs = (const FamilySubtable *)(uintptr_t)F.subtables;
		int32_t first_value = -1;
		bool maps = false;
		for (uint32_t s = 0; s < F.n_subtables; s++) {
			const FamilySubtable st = subs[s];
			if (st.off >= F.cmap_len)
				continue;
			const Sub d{(const uint8_t *)(uintptr_t)F.cmap + st.off, (uint64_t)F.cmap_len - st.off};
			bool listed;
			const int32_t v = lookup(d, st.format, c, listed);
			if (v >= 0) {
				if (first_value < 0)
					first_value = v;
				maps = maps || listed;
			}
		}
		if (maps) {
			e.found = true;
			e.face = k;
			e.gid = (uint32_t)first_value;
			break;
		}
	}
	return e;
}

// the command slots and leaves of a glyph id inside its font (gid < n_glyph_ids): cmd_off's difference of a command font; of a
// glyf font the leaves of leaf_off, which tile the glyph's slots from 0 in order, so the last one ends them
__device__ void glyph_extent(const FamilyFaceRef &F, uint32_t gid, uint32_t &slots, uint32_t &leaves)
{
	const uint32_t *off = (const uint32_t *)(uintptr_t)F.off;
	const uint32_t a = off[gid], b = off[gid + 1];
	if (F.commands) {
		slots = b - a;
		leaves = 0;
		return;
	}
	leaves = b - a;
	slots = 0;
	if (b > a) {
		const vgsdf_glyf_part *parts = (const vgsdf_glyf_part *)(uintptr_t)F.leaves;
		slots = parts[b - 1].cmd_at + parts[b - 1].cmd_cap;
	}
}

__device__ inline uint32_t varint_len(uint32_t v) { return v < 0x80u ? 1u : v < 0x4000u ? 2u : v < 0x200000u ? 3u : v < 0x10000000u ? 4u : 5u; }

struct Sum3 {
	uint32_t e, s, l;
};
// the workgroup's sums, in every thread
__device__ Sum3 block_sum(Sum3 v, uint32_t (*lds)[3])
{
	for (int d = 32; d >= 1; d >>= 1) {
		v.e += __shfl_xor(v.e, d);
		v.s += __shfl_xor(v.s, d);
		v.l += __shfl_xor(v.l, d);
	}
	const uint32_t w = threadIdx.x >> 6;
	if ((threadIdx.x & 63u) == 0)
		lds[w][0] = v.e, lds[w][1] = v.s, lds[w][2] = v.l;
	__syncthreads();
	Sum3 r{0, 0, 0};
	for (uint32_t j = 0; j < kFamilyThreads / 64; j++)
		r.e += lds[j][0], r.s += lds[j][1], r.l += lds[j][2];
	return r;
}

// an `HVAR` table: every read is asked for here first, against the length the face's record gives
struct Tab {
	const uint8_t *p;
	uint64_t n;
};
__device__ inline bool has(const Tab &t, uint64_t off, uint64_t len) { return off <= t.n && len <= t.n - off; }

// Face::hvar_advance_delta: the advance map's (outer, inner) of the glyph id, row `inner` of ItemVariationData[outer] times the
// factors of its regions; false: no delta.  Byte and be16 / be32 loads from one base, each inside hvar_len.
__device__ bool hvar_delta(const FamilyFaceVar &V, uint32_t gid, float &delta)
{
	const Tab t{(const uint8_t *)(uintptr_t)V.hvar, V.hvar_len};
	uint32_t outer = 0, inner = gid;
	if (V.map_off != 0) {
		const uint64_t m = V.map_off;
		if (!has(t, m, 2))
			return false;
		const uint32_t format = t.p[m], ef = t.p[m + 1];
		if (format > 1 || !has(t, m + 2, format ? 4 : 2))
			return false;
		const uint32_t count = format ? be32(t.p + m + 2) : be16(t.p + m + 2);
		if (count == 0)
			return false;
		const uint32_t entry_size = ((ef >> 4) & 3u) + 1u, idx = gid < count - 1u ? gid : count - 1u;
		const uint64_t at = m + (format ? 6u : 4u) + (uint64_t)entry_size * idx;
		if (!has(t, at, entry_size))
			return false;
		uint32_t n = 0;
		for (uint32_t k = 0; k < entry_size; k++)
			n = (n << 8) | t.p[at + k];
		const uint32_t bits = (ef & 15u) + 1u;
		outer = n >> bits, inner = n & ((1u << bits) - 1u);
		if (outer > 0xFFFFu)
			return false;
	}
	const uint64_t s = V.store_off;
	if (!has(t, s, 8) || outer >= be16(t.p + s + 6) || !has(t, s + 8 + 4ull * outer, 4))
		return false;
	const uint64_t at = s + be32(t.p + s + 8 + 4ull * outer);
	if (!has(t, at, 6))
		return false;
	const uint32_t item_count = be16(t.p + at), words = be16(t.p + at + 2), n_cols = be16(t.p + at + 4);
	// (a LONG_WORDS bit the host had not seen makes `words` larger than n_cols: no delta)
	if (!has(t, at + 6, 2ull * n_cols) || inner >= item_count || words > n_cols)
		return false;
	const uint64_t row = at + 6 + 2ull * n_cols + (uint64_t)inner * (words + n_cols);
	if (!has(t, row, (uint64_t)words + n_cols))
		return false;
	const float *scalars = (const float *)(uintptr_t)V.scalars;
	float d = 0.0f;
	uint64_t p = row;
	for (uint32_t c = 0; c < n_cols; c++) {
		const uint32_t region = be16(t.p + at + 6 + 2ull * c);
		float num;
		if (c < words) {
			num = (float)(int16_t)be16(t.p + p);
			p += 2;
		} else {
			num = (float)(int8_t)t.p[p];
			p += 1;
		}
		d += num * (region < V.n_regions ? scalars[region] : 0.0f);
	}
	delta = d;
	return true;
}

// the first and the second of a pack's elements
template <class A, class... R> __device__ inline A first_of(A a, R...) { return a; }
template <class A, class B> __device__ inline B second_of(A, B b) { return b; }

// VAR: the emit pass over faces some of which are at a position; its further arguments, `const FamilyFaceVar *` and, for faces
// whose advances follow gvar's phantom points, `const FamilyFaceGvar *` behind it, are a pack so that the instantiations without
// them keep the arguments (and with them the kernel descriptor and the name) they have always had
template <bool EMIT, bool VAR = false, class... Var>
__global__ __launch_bounds__(kFamilyThreads) void family_tables_pass(const FamilyFaceRef *faces, uint32_t n_faces, uint32_t *counts,
                                                                       uint32_t *flags, uint32_t n_entries, uint8_t *table, uint32_t plane, Var... var)
{
	const uint32_t group = blockIdx.x;
#include "family_table_pass.inc"
}

// ONE face at MANY positions (vgsdf_families_create_tables): the same text over a second grid dimension, the position.  Position p
// is a family of one face: record p of `faces` (the same cmap, hmtx and subtables, font p's off, leaves and n_glyph_ids), of the
// pack's arrays (the same HVAR bytes and factors p; the phantom pass's slices of position p), the counts and the flag word of
// position p, and tables[p].  A position without a table (refused behind the count pass) emits nothing.
template <bool EMIT, bool VAR = false, class... Var>
__global__ __launch_bounds__(kFamilyThreads) void family_tables_batch_pass(const FamilyFaceRef *faces, uint32_t *counts, uint32_t *flags,
                                                                             const FamilyBatchTable *tables, Var... var)
{
	const uint32_t group = blockIdx.x, position = blockIdx.y;
	constexpr uint32_t n_faces = 1, plane = 0; // (the batched constructors build the BMP)
	faces += position, counts += (size_t)kFamilyCounts * kFamilyGroups * position, flags += position;
	((var += position), ...);
	uint32_t n_entries = 0;
	uint8_t *table = nullptr;
	if (EMIT) {
		const FamilyBatchTable T = tables[position];
		if (T.table == 0)
			return; // (the whole workgroup: nothing waits at a barrier)
		n_entries = T.n_entries, table = (uint8_t *)(uintptr_t)T.table;
	}
#include "family_table_pass.inc"
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_family_tables_count(const vgsdf::FamilyFaceRef *faces, uint32_t n_faces, uint32_t plane, uint32_t *counts, uint32_t *flags, hipStream_t stream)
{
	hipLaunchKernelGGL(vgsdf::family_tables_pass<false>, dim3(vgsdf::kFamilyGroups), dim3(vgsdf::kFamilyThreads), 0, stream, faces, n_faces,
	                   counts, flags, 0u, (uint8_t *)nullptr, plane);
	return (int)hipGetLastError();
}

int vgsdf_family_tables_emit(const vgsdf::FamilyFaceRef *faces, uint32_t n_faces, uint32_t plane, const uint32_t *counts, uint32_t n_entries,
                             uint8_t *table, hipStream_t stream)
{
	hipLaunchKernelGGL(vgsdf::family_tables_pass<true>, dim3(vgsdf::kFamilyGroups), dim3(vgsdf::kFamilyThreads), 0, stream, faces, n_faces,
	                   const_cast<uint32_t *>(counts), (uint32_t *)nullptr, n_entries, table, plane);
	return (int)hipGetLastError();
}

int vgsdf_family_tables_emit_var(const vgsdf::FamilyFaceRef *faces, const vgsdf::FamilyFaceVar *var, uint32_t n_faces, const uint32_t *counts,
                                 uint32_t n_entries, uint8_t *table, hipStream_t stream)
{
	hipLaunchKernelGGL((vgsdf::family_tables_pass<true, true>), dim3(vgsdf::kFamilyGroups), dim3(vgsdf::kFamilyThreads), 0, stream, faces,
	                   n_faces, const_cast<uint32_t *>(counts), (uint32_t *)nullptr, n_entries, table, 0u, var);
	return (int)hipGetLastError();
}

int vgsdf_family_tables_emit_gvar(const vgsdf::FamilyFaceRef *faces, const vgsdf::FamilyFaceVar *var, const vgsdf::FamilyFaceGvar *gvar,
                                  uint32_t n_faces, const uint32_t *counts, uint32_t n_entries, uint8_t *table, hipStream_t stream)
{
	hipLaunchKernelGGL((vgsdf::family_tables_pass<true, true>), dim3(vgsdf::kFamilyGroups), dim3(vgsdf::kFamilyThreads), 0, stream, faces,
	                   n_faces, const_cast<uint32_t *>(counts), (uint32_t *)nullptr, n_entries, table, 0u, var, gvar);
	return (int)hipGetLastError();
}

int vgsdf_family_tables_batch_count(const vgsdf::FamilyFaceRef *faces, uint32_t n_positions, uint32_t *counts, uint32_t *flags, hipStream_t stream)
{
	hipLaunchKernelGGL(vgsdf::family_tables_batch_pass<false>, dim3(vgsdf::kFamilyGroups, n_positions), dim3(vgsdf::kFamilyThreads), 0, stream,
	                   faces, counts, flags, (const vgsdf::FamilyBatchTable *)nullptr);
	return (int)hipGetLastError();
}

int vgsdf_family_tables_batch_emit(const vgsdf::FamilyFaceRef *faces, const vgsdf::FamilyFaceVar *var, const vgsdf::FamilyFaceGvar *gvar,
                                   uint32_t n_positions, const uint32_t *counts, const vgsdf::FamilyBatchTable *tables, hipStream_t stream)
{
	const dim3 grid(vgsdf::kFamilyGroups, n_positions), block(vgsdf::kFamilyThreads);
	uint32_t *c = const_cast<uint32_t *>(counts), *no_flags = nullptr;
	if (gvar)
		hipLaunchKernelGGL((vgsdf::family_tables_batch_pass<true, true>), grid, block, 0, stream, faces, c, no_flags, tables, var, gvar);
	else if (var)
		hipLaunchKernelGGL((vgsdf::family_tables_batch_pass<true, true>), grid, block, 0, stream, faces, c, no_flags, tables, var);
	else
		hipLaunchKernelGGL((vgsdf::family_tables_batch_pass<true>), grid, block, 0, stream, faces, c, no_flags, tables);
	return (int)hipGetLastError();
}

} // extern "C"
