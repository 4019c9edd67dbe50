// glyf_table_kernels.hip — a `glyf` face's leaves and simple-entry bytes from its `loca` and `glyf` tables (glyf_table_kernels.h).
// What a lane does for its glyph id is, step for step, Face::resident_table's share for that glyph id (host/ttf_face.cpp):
// Face::glyph_data's loca rules, GlyfWalker::walk's header rules and component records, PartShape::measure at every simple
// entry, Affine::then in f32 (this unit is built with -ffp-contract=off) and ResidentSink::part's fields.  The recursion is a
// loop over an explicit stack in LDS ([level][word][lane]: indexed at run time, so not a private array); the composite being
// read lives in registers.  Every read is bounded by loca_entries / glyf_len, every store of the emit pass by the ranges the
// count pass of the same text has sized.  A glyph id reads at most VGSDF_GLYF_MAX_COMPONENTS component records.
// The walk itself is glyf_table_walk.inc, the body of two pairs of kernels: glyf_tables_pass over one face that comes in the
// kernel's arguments (vgsdf_font_create_tables), glyf_tables_batch_pass over the faces of a batch, each workgroup finding its
// face's record in device memory (vgsdf_fonts_create_tables).
#include "glyf_table_kernels.h"

#include "glyf_table_limits.h"

namespace vgsdf {
namespace {

__device__ inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
__device__ inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
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

// Face::glyph_data: the glyph id's range [a, b) of glyf, or false
__device__ inline bool glyph_range(const GlyfTablesRef &F, uint32_t gid, uint32_t &a, uint32_t &b)
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

// PartShape::measure over body[0, size): the entry behind its 10-byte header
enum ShapeKind : uint32_t { SHAPE_FAIL, SHAPE_NOTHING, SHAPE_PART };
struct Shape {
	ShapeKind kind;
	uint32_t cur, ends, arrays, n_points; // cur: first byte behind the instructions; ends / arrays: bytes that are stored
};
__device__ inline Shape measure(const uint8_t *body, uint32_t size, uint32_t n_contours)
{
	Shape s{SHAPE_FAIL, 0, 0, 0, 0};
	if (n_contours * 2 > size)
		return s;
	const uint32_t last_end = be16(body + (n_contours - 1) * 2);
	if (last_end == 0xFFFFu)
		return s;
	s.n_points = last_end + 1;
	if (s.n_points == 1) {
		s.kind = SHAPE_NOTHING;
		return s;
	}
	uint32_t cur = n_contours * 2;
	if (size - cur < 2)
		return s;
	cur += 2 + be16(body + cur);
	if (cur > size)
		return s;
	const bool fits = n_contours * 2 + (size - cur) <= vg::kGlyfMaxEntry;
	s.kind = SHAPE_PART;
	s.cur = cur;
	s.ends = fits ? n_contours * 2 : 0;
	s.arrays = fits ? size - cur : 0;
	return s;
}

template <bool EMIT>
__global__ __launch_bounds__(kGlyfTableLanes) void glyf_tables_pass(GlyfTablesRef F, uint32_t *counts, const uint32_t *leaf_off,
                                                                     const uint32_t *byte_at, uint32_t *leaves, uint8_t *bytes,
                                                                     uint32_t *flags)
{
	__shared__ uint32_t stack[kGlyfTableLevels][kGlyfTableFrameWords][kGlyfTableLanes];
	const uint32_t lane = threadIdx.x, gid = blockIdx.x * kGlyfTableLanes + lane;
#include "glyf_table_walk.inc"
}

// The same walk over all faces of a batch in one launch (vgsdf_fonts_create_tables).  A workgroup belongs to one face: the LAST
// record f with first_block[f] <= blockIdx.x, found by a bisection every lane runs alike (the records are read through the
// scalar cache).  A face that owns no workgroup — no glyph ids, or not taking part in this pass — has the first_block of the
// face behind it and is passed over by that rule wherever it stands.  Every read stays inside the face's own loca_entries and
// glyf_len; counts and byte_at are the batch's arrays at the face's glyph_base (byte_at: + f, one entry more per face), flags the
// face's own GLYF_FLAG_WORDS words; leaves, bytes and leaf_off lie in the face's own store.
template <bool EMIT>
__global__ __launch_bounds__(kGlyfTableLanes) void glyf_tables_batch_pass(const GlyfFaceRecord *__restrict__ faces, uint32_t n_faces,
                                                                           uint32_t *counts, const uint32_t *byte_at, uint32_t *flags)
{
	__shared__ uint32_t stack[kGlyfTableLevels][kGlyfTableFrameWords][kGlyfTableLanes];
	uint32_t lo = 0, hi = n_faces; // faces[lo].first_block <= blockIdx.x < faces[hi].first_block (faces[0].first_block == 0)
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (faces[mid].first_block <= blockIdx.x)
			lo = mid;
		else
			hi = mid;
	}
	const GlyfFaceRecord &R = faces[lo];
	const uint32_t gid = (blockIdx.x - R.first_block) * kGlyfTableLanes + threadIdx.x;
	if (!R.takes_part) // (never: the host lays the grid over the faces that take part)
		return;
	GlyfTablesRef F;
	F.loca = (const uint8_t *)(uintptr_t)R.loca, F.glyf = (const uint8_t *)(uintptr_t)R.glyf;
	F.glyf_len = R.glyf_len, F.loca_entries = R.loca_entries, F.loca_long = R.loca_long, F.n_glyph_ids = R.n_glyph_ids;
	uint8_t *store = (uint8_t *)(uintptr_t)R.store;
	uint32_t *const leaves = (uint32_t *)store;
	uint8_t *const bytes = store + R.bytes_at;
	const uint32_t *const leaf_off = (const uint32_t *)(store + 16 * (size_t)R.leaf_off_at16);
	const uint32_t lane = threadIdx.x;
	counts += (size_t)kGlyfTableCounts * R.glyph_base, byte_at += R.glyph_base + lo, flags += (size_t)GLYF_FLAG_WORDS * lo;
#include "glyf_table_walk.inc"
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_glyf_tables_count(const vgsdf::GlyfTablesRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + vgsdf::kGlyfTableLanes - 1) / vgsdf::kGlyfTableLanes;
	hipLaunchKernelGGL(vgsdf::glyf_tables_pass<false>, dim3(groups), dim3(vgsdf::kGlyfTableLanes), 0, stream, *face, counts,
	                   (const uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint8_t *)nullptr, flags);
	return (int)hipGetLastError();
}

int vgsdf_glyf_tables_emit(const vgsdf::GlyfTablesRef *face, const uint32_t *leaf_off, const uint32_t *byte_at, void *leaves,
                           uint8_t *bytes, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + vgsdf::kGlyfTableLanes - 1) / vgsdf::kGlyfTableLanes;
	hipLaunchKernelGGL(vgsdf::glyf_tables_pass<true>, dim3(groups), dim3(vgsdf::kGlyfTableLanes), 0, stream, *face, (uint32_t *)nullptr,
	                   leaf_off, byte_at, (uint32_t *)leaves, bytes, flags);
	return (int)hipGetLastError();
}

int vgsdf_glyf_tables_batch_count(const vgsdf::GlyfFaceRecord *faces, uint32_t n_faces, uint32_t n_blocks, uint32_t *counts, uint32_t *flags,
                                  hipStream_t stream)
{
	hipLaunchKernelGGL(vgsdf::glyf_tables_batch_pass<false>, dim3(n_blocks), dim3(vgsdf::kGlyfTableLanes), 0, stream, faces, n_faces, counts,
	                   (const uint32_t *)nullptr, flags);
	return (int)hipGetLastError();
}

int vgsdf_glyf_tables_batch_emit(const vgsdf::GlyfFaceRecord *faces, uint32_t n_faces, uint32_t n_blocks, const uint32_t *byte_at,
                                 uint32_t *flags, hipStream_t stream)
{
	hipLaunchKernelGGL(vgsdf::glyf_tables_batch_pass<true>, dim3(n_blocks), dim3(vgsdf::kGlyfTableLanes), 0, stream, faces, n_faces,
	                   (uint32_t *)nullptr, byte_at, flags);
	return (int)hipGetLastError();
}

} // extern "C"
