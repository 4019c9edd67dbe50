// resident_command_store.h — what the builders of command stores share (resident_fonts.cpp: vgsdf_font_create_commands;
// resident_charstrings.cpp; resident_gvar.cpp): the staging of the context pass beside a store, the function that finishes a
// store, and the running sums that lay a store out from the counts of a count pass, with the bound of its 32-bit offsets.
#pragma once
#include "outline_kernels.h"
#include "resident_build.h"

static_assert(sizeof(vgsdf::OutlineCmd) == 28, "the records of CommandStoreLayout");

// a command font's three arrays, once its store is allocated
inline void name_command_store(vgsdf_font &f, const vgsdf::CommandStoreLayout &at, uint32_t n_cmds)
{
	uint8_t *d = (uint8_t *)f.store.p;
	f.n_cmds = n_cmds;
	f.cref.cmds = (uintptr_t)d, f.cref.cmd_off = (uintptr_t)(d + at.cmd_off), f.cref.open = (uintptr_t)(d + at.open);
}

// what 32-bit offsets address: a store of `cmds` commands over n glyph ids and `floats` coordinates
inline bool command_store_addressable(size_t n, uint64_t cmds, uint64_t floats)
{
	return vgsdf::CommandStoreLayout(n, cmds).total <= 0xFFFFFFFCull && 4ull * floats <= 0xFFFFFFFCull;
}
// ... and what a constructor that counts on the device says of a face past it, behind its own name
constexpr const char *kCommandStorePast = "a store (29 bytes per command, 4 per glyph id) or coordinates past what 32-bit offsets address";

// The store's layout from the counts of a count pass: what vgsdf_font_create_commands is given by its caller.  counts: `stride`
// words per glyph id, the commands in column `cmds_at`, the coordinates in column `floats_at`
struct VGSDF_INTERNAL CommandSums {
	std::vector<uint32_t> cmd_off, dat_off, slots; // [n + 1], [n + 1], [n]: a font's `slots`
	uint32_t n_cmds = 0, n_floats = 0;
	// false: not command_store_addressable
	bool fill(const uint32_t *counts, uint32_t n, uint32_t stride, uint32_t cmds_at, uint32_t floats_at)
	{
		cmd_off.assign((size_t)n + 1, 0), dat_off.assign((size_t)n + 1, 0), slots.assign(n, 0);
		uint64_t cmds = 0, floats = 0;
		for (uint32_t g = 0; g < n; g++) {
			const uint32_t *c = counts + (size_t)stride * g;
			cmd_off[g] = (uint32_t)cmds, dat_off[g] = (uint32_t)floats;
			slots[g] = c[cmds_at];
			cmds += c[cmds_at], floats += c[floats_at];
			if (!command_store_addressable(n, cmds, floats))
				return false;
		}
		cmd_off[n] = n_cmds = (uint32_t)cmds, dat_off[n] = n_floats = (uint32_t)floats;
		return true;
	}
};

// what the packed form's context pass reads beside a command store, for the duration of the call that builds it:
// scale f64[n] (1: the bytes then say "ring open" and nothing else) | dat_off u32[n + 1] | coords | kinds | pad to 16 | its error word
struct ContextStagingLayout {
	size_t scale = 0, dat_off, coords, kinds, flag, total;
	constexpr ContextStagingLayout(size_t n, size_t n_cmds, size_t n_floats)
	    : dat_off(8 * n), coords(dat_off + 4 * (n + 1)), kinds(coords + 4 * n_floats), flag((kinds + n_cmds + 15) / 16 * 16), total(flag + 16)
	{
	}
};
static_assert(ContextStagingLayout(3, 5, 14).kinds == 24 + 16 + 56 && ContextStagingLayout(3, 5, 14).flag == 112 &&
                  ContextStagingLayout(3, 16, 14).flag == 112 && ContextStagingLayout(1, 0, 0).flag == 16 && ContextStagingLayout(1, 0, 0).total == 32,
              "scale | dat_off | coords | kinds | pad to 16 | flag");

// Every single-store constructor, once store (`at`) and staging (t, `tat`) are allocated: uploads cmd_off into the store and the unit
// scales and dat_off into the staging, lets `fill` put kinds and coordinates there (a copy, or the emit pass), runs the context
// pass over them and ends the call's work on the device.  Returns the pass's error word (0 also when q has failed); more_flags (may
// be NULL): a word of the emit pass's to read back with it, from d_more_flags
template <class Fill>
uint32_t finish_command_store(Calls &q, vgsdf_font &f, const vgsdf::CommandStoreLayout &at, uint8_t *t, const ContextStagingLayout &tat,
                              uint32_t n_cmds, const uint32_t *cmd_off, const uint32_t *dat_off, Fill fill, uint32_t *more_flags = nullptr,
                              const void *d_more_flags = nullptr)
{
	const uint32_t n = f.n_glyph_ids;
	uint8_t *d = (uint8_t *)f.store.p;
	const std::vector<double> ones(n, 1.0);
	q.copy(d + at.cmd_off, cmd_off, 4 * ((size_t)n + 1));
	q.copy(t + tat.scale, ones.data(), 8 * (size_t)n);
	q.copy(t + tat.dat_off, dat_off, 4 * ((size_t)n + 1));
	q.zero(t + tat.flag, 16);
	fill();
	if (n_cmds)
		q.launch([&] {
			return vgsdf_outline_context_packed(t + tat.kinds, (const float *)(t + tat.coords), (const uint32_t *)(t + tat.dat_off),
			                                    (const uint32_t *)(d + at.cmd_off), (const double *)(t + tat.scale), n, (vgsdf::OutlineCmd *)d,
			                                    d + at.open, (uint32_t *)(t + tat.flag), q.st);
		});
	uint32_t flag = 0;
	q.read_back(&flag, t + tat.flag, 4);
	if (more_flags)
		q.read_back(more_flags, d_more_flags, 4);
	q.sync();
	name_command_store(f, at, n_cmds);
	return flag;
}
