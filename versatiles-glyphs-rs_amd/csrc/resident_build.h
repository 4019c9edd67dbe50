// resident_build.h — what the constructors of resident fonts (resident_fonts.cpp, resident_charstrings.cpp, resident_glyf_tables.cpp,
// resident_gvar.cpp) and families (resident_families.cpp) share: their error text, what a description of loca and glyf must hold,
// device memory for one call, the sequence of HIP calls of a phase and the events around a count and an emit pass.
// Every allocation here and there asks for 16 bytes more than its layout states, as the front-end's buffers do: a kernel that
// moves a buffer in 16-byte units may touch the whole unit its last byte lies in.  The layouts (upload_layout.h) do not count them.
#pragma once
#include "resident_fonts.h"

// a failed HIP call of a constructor: the entry point's name, what it was doing and the runtime's words
VGSDF_INTERNAL inline int font_hip_error(vgsdf_ctx *ctx, const char *entry, const char *what, hipError_t e)
{
	ctx->err = std::string(entry) + ": " + what + ": " + hipGetErrorString(e);
	return e == hipErrorOutOfMemory ? VGSDF_E_OOM : VGSDF_E_HIP;
}

// a glyf font's three arrays, once its store is allocated
inline void name_glyf_store(vgsdf_font &f, const vgsdf::GlyfStoreLayout &at)
{
	const uintptr_t d = (uintptr_t)f.store.p;
	f.ref.leaves = d + at.leaves, f.ref.bytes = d + at.bytes, f.ref.leaf_off = d + at.leaf_off;
}

// A face's loca and glyf as a constructor is given them (resident_glyf_tables.cpp, resident_gvar.cpp): both tables there ...
inline bool tables_given(const vgsdf_font_tables_desc &in) { return !((in.n_loca_bytes && !in.loca) || (in.n_glyf_bytes && !in.glyf)); }
// ... and a description that can be stated.  (Tables of 4 GiB or more cannot: the lengths are 32-bit.  loca_entries <= num_glyphs + 1:
// every glyph id a component can resolve to is then one of the face's, with a place in the store)
inline bool tables_stateable(const vgsdf_font_tables_desc &in)
{
	return !(in.num_glyphs > 0xFFFFu || in.loca_long > 1u || (uint64_t)in.loca_entries * (in.loca_long ? 4u : 2u) > in.n_loca_bytes ||
	         in.loca_entries > in.num_glyphs + 1);
}

struct VGSDF_INTERNAL ScratchBuf : DevBuf { // device memory for the duration of one call
	~ScratchBuf() { release(); }
};

// resident_gvar.cpp: the phantom pass over one placed glyf face (gvar_advance_kernels.h).  _described: vgsdf_font_create_gvar's
// validation of the description (VGSDF_E_ARG and the context's error text otherwise; num_glyphs is then at most 65535);
// _on_device, over such a description: the pass into `out` — device memory of gvar_advance_bytes(num_glyphs), the f32 delta per
// glyph id at 0, the state byte per glyph id at gvar_advance_state_at(num_glyphs) — complete when the call returns
VGSDF_INTERNAL int gvar_advance_described(vgsdf_ctx *ctx, const char *entry, const vgsdf_font_gvar_desc *desc);
VGSDF_INTERNAL size_t gvar_advance_bytes(uint32_t n_glyph_ids);
VGSDF_INTERNAL size_t gvar_advance_state_at(uint32_t n_glyph_ids);
VGSDF_INTERNAL int gvar_advance_on_device(vgsdf_ctx *ctx, const char *entry, const vgsdf_font_gvar_desc *desc, uint8_t *out, float *ms);

// ... and over one placed glyf face at MANY positions (gvar_advance_batch_kernels.h): the same trio over vgsdf_fonts_gvar_desc
// (n_positions 1 .. VGSDF_FAMILY_MAX_POSITIONS), one launch over (glyph id, position) pairs; `out` holds delta [n_positions x
// num_glyphs] f32 at 0 and the state bytes at gvar_advance_batch_state_at, position after position
VGSDF_INTERNAL int gvar_advance_batch_described(vgsdf_ctx *ctx, const char *entry, const vgsdf_fonts_gvar_desc *desc);
VGSDF_INTERNAL size_t gvar_advance_batch_bytes(uint32_t n_glyph_ids, uint32_t n_positions);
VGSDF_INTERNAL size_t gvar_advance_batch_state_at(uint32_t n_glyph_ids, uint32_t n_positions);
VGSDF_INTERNAL int gvar_advance_batch_on_device(vgsdf_ctx *ctx, const char *entry, const vgsdf_fonts_gvar_desc *desc, uint8_t *out, float *ms);

// The calls of a constructor on its stream, in order, up to the first that fails: after it nothing more is issued, and the
// caller hands `e` to font_hip_error under the name of the phase it is in.  A constructor ends with sync(): its store is complete
// on the device when the call returns, so every context may name the font or family.
struct VGSDF_INTERNAL Calls {
	hipStream_t st;
	hipError_t e = hipSuccess;
	explicit Calls(hipStream_t stream) : st(stream) {}
	bool failed() const { return e != hipSuccess; }
	// host to device; nothing for no bytes
	void copy(void *dst, const void *src, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); }
	void zero(void *dst, size_t bytes) { if (e == hipSuccess) e = hipMemsetAsync(dst, 0, bytes, st); }
	// f() returns hipError_t or a kernel launcher's int; it is not called once a call has failed
	template <class F> void launch(F &&f) { if (e == hipSuccess) e = (hipError_t)f(); }
	void record(hipEvent_t ev) { if (e == hipSuccess) e = hipEventRecord(ev, st); }
	void read_back(void *dst, const void *src, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); }
	void sync() { if (e == hipSuccess) e = hipStreamSynchronize(st); }
};

// what an exported `…_kernel_ms` getter answers: the context's pair of the last call, zeros without a context
inline void pass_ms_out(const float *pair, float ms[2])
{
	if (ms)
		ms[0] = pair ? pair[0] : 0.0f, ms[1] = pair ? pair[1] : 0.0f;
}

// the events around a count pass (0 .. 1) and an emit pass (1 .. 2; the emit pass records 1 again), and their times for the
// context's `…_ms` pair
struct VGSDF_INTERNAL PassEvents {
	hipEvent_t at[3] = {nullptr, nullptr, nullptr};
	hipError_t create()
	{
		for (hipEvent_t &ev : at)
			if (hipError_t err = hipEventCreate(&ev); err != hipSuccess)
				return err;
		return hipSuccess;
	}
	void elapsed(float ms[2], int pass) const { (void)hipEventElapsedTime(&ms[pass], at[pass], at[pass + 1]); } // behind a sync()
	~PassEvents()
	{
		for (hipEvent_t ev : at)
			if (ev)
				(void)hipEventDestroy(ev);
	}
};
