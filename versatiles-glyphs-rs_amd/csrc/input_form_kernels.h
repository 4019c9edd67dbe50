// input_form_kernels.h — launchers of input_form_kernels.hip: how a submission's commands come to be on the device.
#pragma once
#include "outline_kernels.h"

extern "C" {
// the decoder's limits per part (kGlyfMaxPoints, kGlyfMaxBytes: beyond them a part fails with error_flag bit 4) and the number of
// font references a workgroup of the resident upload keeps in LDS (kExpandFontCache); any pointer may be NULL.  For tests that
// restate the constants (as vgsdf_filtered_delta_cap): not part of the public ABI of include/
void vgsdf_glyf_limits(uint32_t *max_points, uint32_t *max_bytes, uint32_t *expand_font_cache);
// parts: vgsdf_glyf_part records (include/vgsdf.h); writes the commands of every part into its slots of `cmds`;
// error_flag bit 4: a malformed entry
// max_cmd_cap / max_byte_len: the largest cmd_cap / byte_len among the parts (they size the launch's LDS)
// cmd_open (may be NULL): the context pass's byte per command, written by the decoder itself — only for batches whose scales
// are all positive and finite (bit 1 of that byte is never set here)
int vgsdf_glyf_decode(const void *parts, uint32_t n_parts, const uint8_t *bytes, vgsdf::OutlineCmd *cmds, uint32_t *error_flag,
                      uint32_t max_cmd_cap, uint32_t max_byte_len, uint8_t *cmd_open, hipStream_t stream);
// the same for parts expanded from resident fonts: fonts = vgsdf::ResidentFontRef records (upload_layout.h), a part's font
// index in the upper half of its `plain`
int vgsdf_glyf_decode_resident(const void *parts, uint32_t n_parts, const void *fonts, vgsdf::OutlineCmd *cmds, uint32_t *error_flag,
                               uint32_t max_cmd_cap, uint32_t max_byte_len, uint8_t *cmd_open, hipStream_t stream);
// upload of a vgsdf_outlines_resident submission: copies the block (ResidentBlockLayout, padded to 16 bytes; src: the device
// address of the page-locked block, or a device copy of it) to dst and expands the glyphs' leaves into parts_out[n_parts]
int vgsdf_resident_expand(const void *src, void *dst, size_t block_bytes, uint32_t n_glyphs, uint32_t n_parts, uint32_t n_fonts,
                          bool with_pbf, void *parts_out, hipStream_t stream);
// upload of a vgsdf_outlines_resident submission against command fonts: copies the block (CommandBlockLayout, padded to 16
// bytes; src as above) to dst and gathers the named glyphs' records and context bytes from the fonts' stores
// (vgsdf::CommandFontRef records in the block) into cmds_out[n_cmds] / cmd_open[n_cmds] at the block's cmd_off
int vgsdf_resident_gather(const void *src, void *dst, size_t block_bytes, uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_fonts,
                          bool with_pbf, vgsdf::OutlineCmd *cmds_out, uint8_t *cmd_open, hipStream_t stream);
// upload of a vgsdf_outlines_submit_resident_mixed submission, fonts of both kinds in one list: copies the block
// (ResidentBlockLayout, its font references vgsdf::MixedFontRef records that say their kind) to dst, expands the leaves of the
// glyphs of glyf fonts into parts_out[n_parts] and gathers the records and context bytes of the glyphs of command fonts into
// cmds_out / cmd_open at the block's cmd_off; the slots of the glyf glyphs are left to the decoder
int vgsdf_resident_mixed(const void *src, void *dst, size_t block_bytes, uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_parts, uint32_t n_fonts,
                         bool with_pbf, void *parts_out, vgsdf::OutlineCmd *cmds_out, uint8_t *cmd_open, hipStream_t stream);
// the kinds of font list an upload kernel of a named form is stamped for
enum { VGSDF_FONTS_GLYF = 0, VGSDF_FONTS_COMMANDS = 1, VGSDF_FONTS_MIXED = 2 };
// upload of a vgsdf_outlines_ranges submission, against fonts of either kind or (VGSDF_FONTS_MIXED: both arrays written) of both: src = the block (upload_layout.h,
// RangesBlockLayout: n_tasks task records, n_families family records, n_fonts font references; device-readable as above),
// dst = the device's copy in ResidentBlockLayout / CommandBlockLayout, whose per-glyph arrays and font references the kernel
// WRITES; then the expansion into parts_out[n_parts] (glyf fonts) or the gather into cmds_out / cmd_open[n_cmds] (command
// fonts).  names: vgsdf::EntryName[n_glyphs], written when with_pbf (for vgsdf_pbf_entries).  error_flag bit 5: an index of the
// block that does not hold against these counts
int vgsdf_family_upload(int kind, const void *src, void *dst, uint32_t n_glyphs, uint32_t n_cmds, uint32_t n_parts, uint32_t n_fonts,
                        uint32_t n_tasks, uint32_t n_families, bool with_pbf, void *parts_out, vgsdf::OutlineCmd *cmds_out,
                        uint8_t *cmd_open, void *names, uint32_t *error_flag, hipStream_t stream);
// upload by a kernel: src_mapped = device address of a page-locked, device-mapped host block (16-byte aligned), dst 16-byte aligned
int vgsdf_copy_in(const void *src_mapped, void *dst, size_t bytes, hipStream_t stream);
}
