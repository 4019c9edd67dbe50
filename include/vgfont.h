/*
 * vgfont.h — flat C view of the C++ host façade in libvgsdf.so (namespace vg):
 * FontManager / GlyphBlock / Renderer with the reference's names and semantics, driving
 * the GPU raster of vgsdf.h.  Replaces, for the render path only:
 *   FontManager::{new,add_font_with_name,render_glyphs}  /root/reference/src/font/manager.rs:28,66,81
 *   FontManager::{add_path,add_paths}, scan              manager.rs:39-61, src/commands/recurse.rs:104-133
 *   write_index_json / write_families_json               manager.rs:128-138, src/font/index_files.rs:65-143
 *   Writer::{new_tar,new_file}                           src/writer/mod.rs:27-41, tar.rs:30-157, file.rs:10-52
 *   parse_font_name / FontMetadata::generate_name        src/font/parse_font_name.rs:214-291, metadata.rs:43-68
 *   GlyphBlock::render                                   src/font/glyph_block.rs:69
 *   Renderer::{new,new_precise,new_dummy,render_glyph}   src/render/renderer.rs:25-43,103
 * This header exists so tests/bench (Python ctypes) and non-C++ callers can reach the
 * façade; C++ callers include csrc/host/font_manager.hpp directly.
 *
 * Return convention: >= 0 success, < 0 failure with the message in vg_last_error()
 * (thread-local).  Renderer mode VG_MODE_HIP has no CPU fallback.
 */
#ifndef VGFONT_H
#define VGFONT_H
#include <stddef.h>
#include <stdint.h>

#include "vgsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vg_manager vg_manager;
typedef struct vg_renderer vg_renderer;
typedef struct vg_glyph_batch vg_glyph_batch;

enum { VG_MODE_HIP = 0, VG_MODE_DUMMY = 1 }; /* renderer.rs:14-17 RendererMode {Precise,Dummy} */

/* PbfGlyph (src/protobuf/glyph.rs:10-41) without the pixels */
typedef struct {
	uint32_t id;
	int32_t has_bitmap;
	uint32_t width, height;
	int32_t left, top;
	uint32_t advance;
	uint32_t bitmap_len;
} vg_pbf_glyph;

/* phases of the last vg_manager_render_glyphs call */
typedef struct {
	double tessellate_s, pack_s, device_s, encode_s, write_s, total_s;
	uint64_t blocks, glyphs, rasters, pixels, segments, pbf_bytes;
	uint64_t glyf_groups;    /* submissions whose glyphs the device decoded from their `glyf` arrays */
	uint64_t glyf_fallbacks; /* of which the device refused (a malformed entry) and the host's reader recorded again */
	uint64_t fe_groups;           /* groups of the dispatcher that held glyphs (one device submission each) */
	uint64_t fe_max_group_glyphs; /* glyphs of the largest of those groups */
} vg_timings;

/* Writer sink (src/writer/mod.rs:10-19): is_dir=1 for write_directory. Return 0, or
 * non-zero to abort the render (first error aborts, manager.rs:117-121). */
typedef int (*vg_write_cb)(void *user, const char *path, const uint8_t *data, size_t len, int is_dir);

const char *vg_last_error(void);

vg_renderer *vg_renderer_new(int mode, int device_ordinal);
/* ONE process, n devices (the reference is one process with a rayon pool, src/font/manager.rs:81-125):
 * a HIP renderer with one lane per entry of `devices` (own device contexts and streams each; an entry may repeat a
 * device).  vg_manager_render_glyphs / _to with such a renderer deal the run's (font, block) tasks — manager.rs:86-97's
 * unit — to the lanes, longest first; every lane renders its tasks on its own host thread and every file comes whole from
 * one lane.  Where whole tasks do not balance (ONE font's 20-45 unequal blocks on 8 devices) the glyphs of the few heaviest
 * blocks are split between lanes and those blocks' partial PBFs merged in this process's memory (the hybrid plan;
 * vg_manager_plan_lanes shows it, vg_manager_set_lane_form chooses another form) — there is no exchange step.  Output bytes
 * equal a single-device run's in every form.  The run
 * counters {blocks, glyphs, pixels} are summed over the lanes with vgsdf_reduce_counters (RCCL all-reduce when the
 * devices are distinct; the host's own sum, flagged in vg_renderer_reduce_path, if RCCL fails) and checked; vg_manager_reduced_counters returns them.  NULL + vg_last_error() on failure. */
vg_renderer *vg_renderer_new_multi(const int *devices, int n);
int vg_renderer_device_count(const vg_renderer *r);
/* sum of the lanes' run counters as they stand (vgsdf_reduce_counters over the renderer's contexts) */
int vg_renderer_reduce_counters(const vg_renderer *r, uint64_t counters[3]);
/* how the last reduce (vg_renderer_reduce_counters, or the one at the end of a multi-lane vg_manager_render_glyphs) took
 * its sum: vgsdf_reduce_path of lane 0 — "rccl", "host: contexts share a device", "host: RCCL fallback: <reason>" ...
 * (valid until the next call on this thread) */
const char *vg_renderer_reduce_path(const vg_renderer *r);
void vg_renderer_add_counters(const vg_renderer *r, int lane, uint64_t blocks, uint64_t glyphs, uint64_t pixels);
void vg_renderer_reset_counters(const vg_renderer *r);
void vg_renderer_free(vg_renderer *r);

vg_manager *vg_manager_new(int parallel);
void vg_manager_free(vg_manager *m);
void vg_manager_set_threads(vg_manager *m, unsigned threads, unsigned blocks_per_batch);
/* 1: flatten / close / scale / bbox on the GPU (device front-end of vgsdf.h; HIP renderer
 * only), 0: on host threads.  Same bytes either way. */
void vg_manager_set_device_front_end(vg_manager *m, int on);
/* Union outlines (rule U; vgsdf_batch_union / vgsdf_outlines_union of vgsdf.h): 1 = every route of the
 * HIP renderer rasters the BOUNDARY of a glyph's filled set instead of its segments, so that the edges of one contour inside
 * another (overlapping contours of variable fonts, accents over their bases) no longer draw a seam through the stroke.  The
 * bitmaps are then deliberately NOT the reference crate's; metrics, advances and PBF framing are.  0 (default): the crate's
 * bytes.  VG_MODE_DUMMY ignores the switch.  Costs the raster fused behind the device front-end's plan.
 * The manager hands the switch to the renderer for the length of a render call: a renderer serves ONE manager's render call
 * at a time (calls one after the other may differ in their switches; two at once on one renderer may not). */
void vg_manager_set_union_outlines(vg_manager *m, int on);
/* what the union pass saw in this manager's runs so far: glyphs seen = rebuilt + identity (nothing to do) + passed through
 * over the limit of 6144 segments + passed through with a coordinate that is not finite.  Any pointer may be NULL. */
void vg_manager_union_stats(const vg_manager *m, uint64_t *seen, uint64_t *rebuilt, uint64_t *identity, uint64_t *over_limit);
/* 1 (default): blocks are assembled IN PLACE — the raster stores every bitmap where its block's finished PBF has it, the
 * host writes the ~20 bytes around it (src/protobuf/glyphs.rs:66-70 without a second copy of the bitmaps); 0: bitmaps
 * packed back to back, blocks encoded afterwards.  Same bytes either way. */
void vg_manager_set_in_place_pbf(vg_manager *m, int on);
/* glyf fonts through the device front-end: 1 (default) = the glyphs' `glyf` arrays are copied as they stand and decoded on
 * the device (vgsdf_outlines_submit_glyf: what ttf-parser's Face::outline_glyph does for renderer.rs:110, replayed there),
 * 0 = the host's reader records the callbacks (CFF / CFF2 fonts always take that way; so does a batch in which the device
 * finds a malformed entry).  Same bytes either way. */
void vg_manager_set_glyf_on_device(vg_manager *m, int on);
/* Resident fonts, 0 (default) / 1.  With 1 a group of the dispatcher whose faces all have `glyf` outlines (and were not
 * refused by the device's decoder before) is submitted by (font, glyph id) — vgsdf_outlines_submit_resident, 33 bytes per
 * glyph — against device copies of the faces that the RENDERER owns: one per (device, face), uploaded on first use,
 * shared by the two contexts of a lane and by the lanes of vg_renderer_new_multi that share a device, freed with the
 * renderer.  Every entry point that runs the dispatcher takes it (vg_manager_render_glyphs, _render_glyphs_to,
 * _render_blocks, every lane form); vg_manager_render_block and vg_render_glyph stay as they are.  A face without a resident
 * form, or one that does not fit the renderer's budget, sends its groups through the glyf form; a malformed entry falls
 * back to the host's reader exactly as there (vg_timings.glyf_fallbacks).  Same bytes either way.
 * vg_renderer_set_resident_budget: HBM the device copies may take per device (default 1 GiB, a setting; no eviction).
 * vg_renderer_preload_fonts: uploads every face of the manager now, for callers that want the first request warm; returns
 * the bytes put on the devices, -1 on error.
 * vg_manager_resident_stats: of the last render. */
void vg_manager_set_resident_fonts(vg_manager *m, int on);
void vg_renderer_set_resident_budget(vg_renderer *r, uint64_t bytes_per_device);
long long vg_renderer_preload_fonts(vg_renderer *r, const vg_manager *m);
typedef struct {
	uint64_t groups;         /* groups submitted in the resident form */
	uint64_t fonts_uploaded; /* faces uploaded during the render */
	uint64_t font_bytes;     /* ... and what they occupy on the device */
	uint64_t block_bytes;    /* bytes of the submissions' upload blocks */
} vg_resident_stats;
int vg_manager_resident_stats(const vg_manager *m, vg_resident_stats *out);
/* Command stores, 0 (default) / 1 / 2, independent of vg_manager_set_resident_fonts.  A command store is a face's outline
 * callbacks by glyph id, expanded once on the device (vgsdf_font_create_commands): every face the reader can read has one.
 * The renderer owns them as it owns the resident fonts — same registry, one per (device, face), same budget, no eviction.
 *   0: nothing changes.
 *   1: a group of the dispatcher that cannot take a glyf form — a face without `glyf` outlines (CFF, CFF2), a font the
 *      device's decoder or the batch bounds have refused — is submitted by (font, glyph id) against command stores of all
 *      its faces instead of being read by the host on every render.  Groups that can take a glyf form are untouched; a group
 *      the device refuses still falls back to the host's reader exactly as before (vg_timings.glyf_fallbacks), and later
 *      groups of that font go by name.
 *   2: every group goes by name against command stores, `glyf` faces included (an A/B lever: no decoder launch, more HBM).
 * A store that does not fit the budget sends its groups the way they go with 0.  Same bytes in every mode.  Every entry point
 * that runs the dispatcher takes it; vg_manager_render_block and vg_render_glyph stay as they are.
 * vg_renderer_preload_fonts also uploads the command stores the manager's mode would use.
 * vg_manager_command_stats: of the last render (vg_resident_stats keeps counting the glyf-resident groups only). */
void vg_manager_set_resident_commands(vg_manager *m, int mode);
typedef struct {
	uint64_t groups;         /* groups submitted by name against command stores */
	uint64_t fonts_uploaded; /* command stores uploaded during the render */
	uint64_t font_bytes;     /* ... and what they occupy on the device */
	uint64_t block_bytes;    /* bytes of those submissions' upload blocks */
} vg_command_stats;
int vg_manager_command_stats(const vg_manager *m, vg_command_stats *out);
/* Mixed stores, 0 (default) / 1; has an effect only with vg_manager_set_glyf_on_device, vg_manager_set_resident_fonts and
 * vg_manager_set_resident_commands(1).  Without it, ONE glyph from a file without `glyf` outlines sends every file of its group's
 * font ids to the command stores — a Noto Sans directory with the CFF CJK files under the same font id has every TrueType file
 * interpreted on the host for that.  With it, stores go per FILE: a face with `glyf` outlines whose glyf store can be made (host
 * table or device builder, batched or not) gets a glyf store, every other face a command store (charstrings on the device where
 * that switch is on), and a group that is not all `glyf` and has at least one glyf store among its files is submitted against
 * both kinds at once: vgsdf_outlines_submit_resident_mixed, or with vg_manager_set_resident_families as ranges of MIXED families
 * (vgsdf_family_create_mixed; _create_tables_mixed with vg_manager_set_family_tables_on_device), which the renderer keeps beside
 * the others under their own key — same budget, lifetime and fallbacks.  A group without a glyf store goes to the command forms
 * exactly as with 0, a group that is all `glyf` to the glyf forms, mode 2 of the command stores is untouched; a group the
 * device refuses falls back to the host's reader as ever (and its font ids get command stores from then on).  Same bytes.
 * vg_renderer_preload_fonts also builds the mixed families when the mode is on.
 * vg_manager_mixed_stats: of the last render; such groups are counted here and in none of vg_family_stats, vg_resident_stats and
 * vg_command_stats, while the stores uploaded for them count in the upload counters of their kind. */
void vg_manager_set_mixed_stores(vg_manager *m, int on);
typedef struct {
	uint64_t groups;        /* groups submitted against stores of both kinds (by name or as ranges of mixed families) */
	uint64_t glyf_fonts;    /* glyf stores those groups named */
	uint64_t command_fonts; /* command stores those groups named */
	uint64_t block_bytes;   /* bytes of those submissions' upload blocks */
} vg_mixed_stats;
int vg_manager_mixed_stats(const vg_manager *m, vg_mixed_stats *out);
/* Charstrings on the device, 0 (default) / 1 / 2.  With 1, wherever the renderer would build the command store of a `CFF ` version 1
 * face — modes 1 and 2 above, vg_renderer_preload_fonts, families — the DEVICE interprets the face's charstrings
 * (vgsdf_font_create_charstrings) instead of the host's reader; the host only resolves the INDEX offsets.  A face the device
 * refuses (a seac glyph, a glyph past VGSDF_CHARSTRING_MAX_TOKENS, a store past the bounds) gets its store from the host reader as with 0.  Same
 * registry, same budget, same store bytes and same output either way.  With 1, CFF2 and `glyf` faces are not affected.  With 2,
 * everything 1 does, and CFF2 faces likewise through vgsdf_font_create_charstrings2, with the blend factors of the host reader
 * (those of the file's position: the default one of the design space unless vg_manager_add_font_instance put it elsewhere); same fallback, same stats.  `glyf` faces are not affected.  Any other non-zero value: 1.
 * vg_manager_charstring_stats: of the last render; the decoded stores count among vg_command_stats.fonts_uploaded too. */
void vg_manager_set_charstrings_on_device(vg_manager *m, int on);
typedef struct {
	uint64_t fonts_decoded; /* command stores the device decoded from charstrings during the render */
	uint64_t font_bytes;    /* their bytes on the device */
	uint64_t fallbacks;     /* faces the device refused: their stores came from the host reader */
} vg_charstring_stats;
int vg_manager_charstring_stats(const vg_manager *m, vg_charstring_stats *out);
/* the same of the manager's last vg_renderer_preload_fonts (its stores are built outside any render) */
int vg_manager_charstring_preload_stats(const vg_manager *m, vg_charstring_stats *out);
/* Resident families, 0 (default) / 1: a group that the two switches above would submit by (font, glyph id) — against resident
 * fonts or command stores — is submitted as code-point ranges of its font ids' families instead (vgsdf_outlines_submit_ranges):
 * one task per (font, block), one per run of code points for a block the hybrid lane plan has split.  The renderer owns the
 * families beside the fonts (same registry, budget and lifetime; rebuilt when a file is added to the font id); recording a
 * group is O(tasks), the device writes the PBF entries and the host only the block headers (in-place PBF off: the bitmaps come
 * packed and the host encodes, id and advance from the family's host table).  A group the device refuses falls back to the
 * host's reader as ever; with glyph sharding on (vg_manager_set_glyph_shard, lane form 0) groups go by glyph names as without
 * the switch.  Same bytes.  vg_renderer_preload_fonts also builds the families when the mode is on.
 * vg_manager_family_stats: of the last render (such groups are counted here, not in the two stats above). */
void vg_manager_set_resident_families(vg_manager *m, int on);
typedef struct {
	uint64_t groups;            /* groups submitted as ranges of families */
	uint64_t families_uploaded; /* families put on a device during the render */
	uint64_t family_bytes;      /* ... and what they occupy there */
	uint64_t block_bytes;       /* bytes of those submissions' upload blocks */
} vg_family_stats;
int vg_manager_family_stats(const vg_manager *m, vg_family_stats *out);
/* Family tables on the device, 0 (default) / 1: wherever the renderer makes a resident family — groups of the switch above,
 * vg_renderer_preload_fonts — the DEVICE builds its table from the faces' `cmap` and `hmtx` tables (vgsdf_family_create_tables);
 * the host only says where the unicode subtables are (vg_manager_family_tables_desc) and looks no code point up.  A font id
 * whose description refuses (a cmap subtable that is not regular), or whose build the device refuses, gets its family from the
 * host's table as with 0, remembered per font id and device.  Same registry key, budget and lifetime, same table bytes and
 * same output either way.  vg_manager_family_table_stats: of the last render; the families built count among
 * vg_family_stats.families_uploaded too. */
void vg_manager_set_family_tables_on_device(vg_manager *m, int on);
typedef struct {
	uint64_t built_on_device; /* families whose tables the device built during the render */
	uint64_t fallbacks;       /* font ids whose families came from the host's table although the switch is on */
} vg_family_table_stats;
int vg_manager_family_table_stats(const vg_manager *m, vg_family_table_stats *out);
/* ... and of the families of the supplementary planes (vg_manager_set_supplementary_planes; of the last render).  With the switch
 * above on, a STATIC font id's supplementary families are built by the device (vgsdf_family_create_tables_at), the planes chosen by
 * ONE vgsdf_family_tables_census call per font id — a plane whose bits are all clear is not built on the device; the host's block
 * table remains the authority for what is written.  A font id with a placed face (an fvar instance), or with the switch off, or
 * whose build was refused, takes vgsdf_family_create_at from the host's table.  built_on_device counts among
 * vg_family_table_stats.built_on_device too. */
typedef struct {
	uint64_t census_calls;    /* vgsdf_family_tables_census calls */
	uint64_t built_on_device; /* supplementary families the device built */
	uint64_t stated_by_host;  /* supplementary families stated by the host through vgsdf_family_create_at */
	uint64_t planes;          /* bit p: a family of plane p (1 .. 16) was made, either way */
} vg_family_plane_stats;
int vg_manager_family_plane_stats(const vg_manager *m, vg_family_plane_stats *out);
/* Glyf tables on the device, 0 (default) / 1: wherever the renderer makes a glyf-kind resident font — glyph-named groups, the
 * families, vg_renderer_preload_fonts — the DEVICE walks the face's `loca` and `glyf` tables (vgsdf_font_create_tables); the host
 * only says where the tables are (vg_manager_font_tables_desc) and interprets no glyph.  A face whose build the device refuses
 * (a glyph that reads more than 2^20 component records, the bounds of the resident form, a device error) gets its font from the host's table
 * as with 0, remembered per face and device.  Same registry key, budget and lifetime, same leaves and same output either way.
 * vg_manager_glyf_table_stats: of the last render; the fonts built count among vg_resident_stats.fonts_uploaded too. */
void vg_manager_set_glyf_tables_on_device(vg_manager *m, int on);
typedef struct {
	uint64_t built_on_device; /* fonts the device walked from loca and glyf during the render */
	uint64_t bytes;           /* ... and what they occupy there */
	uint64_t fallbacks;       /* faces whose fonts came from the host's table although the switch is on */
} vg_glyf_table_stats;
int vg_manager_glyf_table_stats(const vg_manager *m, vg_glyf_table_stats *out);
/* gvar on the device, 0 (default) / 1: the command store of a `glyf` face placed by vg_manager_add_font_instance is built by the
 * DEVICE from the face's `loca`, `glyf` and `gvar` at the face's coordinates (vgsdf_font_create_gvar: deltas, inferred points and
 * component offsets there); the host only says where the tables are (vg_manager_gvar_font_desc) and interprets no glyph.  A face
 * the device refuses (malformed variation data, a glyph past VGSDF_GVAR_MAX_DELTAS, the walk's and the store's bounds) gets its
 * store from the host reader as with 0, remembered per face and device, so it is tried once.  Same registry key (the face's
 * command serial), budget and lifetime, same store and same output either way.  Off by default whatever a measurement says
 * (profiles/gvar_instances_ab.txt).  vg_manager_gvar_stats: of the last render; the stores built count among
 * vg_command_stats.fonts_uploaded too. */
void vg_manager_set_gvar_on_device(vg_manager *m, int on);
typedef struct {
	uint64_t fonts_built; /* command stores the device built from loca, glyf and gvar during the render */
	uint64_t font_bytes;  /* their bytes on the device */
	uint64_t fallbacks;   /* faces the device refused: their stores came from the host reader */
} vg_gvar_stats;
int vg_manager_gvar_stats(const vg_manager *m, vg_gvar_stats *out);
/* ... batched, 0 (default) / 1; has an effect only with vg_manager_set_gvar_on_device: when the store of a placed `glyf` face
 * that shares its bytes with other placed faces — the instances of vg_manager_add_font_named_instances; files added with
 * vg_manager_add_font_instance keep their own copies and their own calls — is asked for, the stores of ALL faces of that group
 * that the lane's device has yet to build are built in one call (vgsdf_fonts_create_gvar: the tables uploaded once, one count
 * launch, the deltas and the emit pass over all positions), each under its own command serial.  A refused position gets its store
 * from the host reader, counted in vg_gvar_stats.fallbacks and remembered; one past the budget is left unbuilt, as without the
 * switch.  vg_renderer_preload_fonts does the same.  Same stores, registry, budget and vg_gvar_stats, same output.  Off by
 * default whatever a measurement says (profiles/gvar_batch_ab.txt).  vg_manager_gvar_batch_stats: of the last render. */
void vg_manager_set_gvar_batched(vg_manager *m, int on);
typedef struct {
	uint64_t calls; /* batched calls made during the render (a group whose stores were all there makes none) */
	uint64_t faces; /* the faces they were given */
} vg_gvar_batch_stats;
int vg_manager_gvar_batch_stats(const vg_manager *m, vg_gvar_batch_stats *out);
/* CFF2 command stores of all instances of a file in one device build, 0 (default) / 1; has an effect only with
 * vg_manager_set_charstrings_on_device(m, 2): when the command store of a placed CFF2 face that shares its bytes with other placed
 * faces — the instances of vg_manager_add_font_named_instances; files added with vg_manager_add_font_instance keep their own
 * copies and their own calls — is asked for, the stores of ALL faces of that group that the lane's device lacks and that are not
 * remembered as refused or as not fitting are built in one call (vgsdf_fonts_create_charstrings2_within: the charstrings uploaded
 * once, the count and the emit pass over all positions), each under its own command serial.  A refused position gets its store
 * from the host reader, counted in vg_charstring_stats.fallbacks and remembered; one past the budget is left unbuilt, as without
 * the switch.  vg_renderer_preload_fonts and the batched family path do the same.  Same stores, registry, budget and
 * vg_charstring_stats, same output.  Off by default whatever a measurement says (profiles/charstrings2_batch_ab.txt).
 * vg_manager_charstring_batch_stats: of the last render. */
void vg_manager_set_charstrings_batched(vg_manager *m, int on);
typedef struct {
	uint64_t calls; /* batched calls made during the render (a group whose stores were all there makes none) */
	uint64_t faces; /* the faces they were given */
} vg_charstring_batch_stats;
int vg_manager_charstring_batch_stats(const vg_manager *m, vg_charstring_batch_stats *out);
/* family tables of all instances of a file in one device build, 0 (default) / 1; has an effect only with
 * vg_manager_set_family_tables_on_device: when the family of a font id whose ONE file is a placed face that shares its bytes
 * with other placed faces — the instances of vg_manager_add_font_named_instances, `glyf` + `gvar` and CFF2 alike — is asked
 * for, the stores of the group's faces are made as today and the family tables of ALL its single-file font ids that the lane's
 * device lacks are built in one call (vgsdf_families_create_tables: cmap, hmtx and HVAR or loca, glyf and gvar uploaded once,
 * one phantom pass, one count and one emit pass over all positions), each under its own family's serial.  A refused position is
 * remembered and gets its table the host's way, counted as any family-table fallback.  A font id of several files (two records
 * merged into one id), a group of one and a family past the budget stay on the single path.  vg_renderer_preload_fonts is not
 * touched.  Same families, registry, budget and family-table stats, same output.  Off by default whatever a measurement says
 * (profiles/family_batch_ab.txt).  vg_manager_family_batch_stats: of the last render. */
void vg_manager_set_family_tables_batched(vg_manager *m, int on);
typedef struct {
	uint64_t calls;    /* batched calls made during the render (a group whose families were all there makes none) */
	uint64_t families; /* the families they made */
} vg_family_batch_stats;
int vg_manager_family_batch_stats(const vg_manager *m, vg_family_batch_stats *out);
/* advances from gvar's phantom points, 0 (default) / 1: a `glyf` + `gvar` face placed AFTER the call — by
 * vg_manager_add_font_instance, _normalized, vg_manager_add_font_named_instances or the named-instance scan — whose file has no
 * readable `HVAR` takes every glyph id's advance from the deltas of phantom points n and n + 1 of its `gvar` data (rule G7 of
 * csrc/host/ttf_face.hpp) instead of keeping `hmtx`'s.  The advance is the PBF entry's and the source of the sub-pixel shift
 * that moves the outline, so entries and bitmaps follow.  A file with a readable `HVAR` is not touched by the switch.  NOT
 * RETROACTIVE: stores and families are keyed by serials taken at placement, so faces placed before the call keep what they had.
 * Everything that asks the reader for an advance follows (the host's family table, record_resident, command tables, the CPU
 * path); nothing else differs from an `HVAR` face: named instances, ranges, mixed families, in-place PBF, lane plans, glyph
 * sharding, gvar on the device and its batched form see only another advance.  With vg_manager_set_family_tables_on_device the
 * faces' loca, glyf and gvar go to the device beside the variation records (vg_manager_family_gvar_desc,
 * vgsdf_family_create_tables_gvar: the phantom pass and the emit pass there); a refusal or device error sends the font id the
 * host's way, counted as any family-table fallback and in `fallbacks` below.  Off by default whatever a measurement says
 * (profiles/gvar_advances_ab.txt). */
void vg_manager_set_gvar_advances(vg_manager *m, int on);
typedef struct {
	uint64_t faces;         /* faces placed so far whose advances follow G7 */
	uint64_t device_builds; /* of the last render: families with such a face that the device built, the phantom pass included */
	uint64_t fallbacks;     /* ... and those it refused, whose tables came from the host reader instead */
} vg_gvar_advance_stats;
int vg_manager_gvar_advance_stats(const vg_manager *m, vg_gvar_advance_stats *out);
/* ... batched, 0 (default) / 1; has an effect only with vg_manager_set_glyf_tables_on_device: the glyf fonts of ALL files of a
 * font id that the device has yet to build are built in one call (vgsdf_fonts_create_tables: one count launch, one read-back, one
 * emit launch) instead of one call per file, so what a call costs beside its two passes is paid once per font id.  Same fonts,
 * same registry, budget, fallbacks and vg_glyf_table_stats, same output.  vg_manager_glyf_table_batch_stats: of the last render. */
void vg_manager_set_glyf_tables_batched(vg_manager *m, int on);
typedef struct {
	uint64_t calls; /* batched calls made during the render (a font id whose fonts were all there makes none) */
	uint64_t faces; /* the faces they were given */
} vg_glyf_table_batch_stats;
int vg_manager_glyf_table_batch_stats(const vg_manager *m, vg_glyf_table_batch_stats *out);
/* How a renderer of several device lanes (vg_renderer_new_multi) splits a run: -1 / 2 (default) the hybrid plan — whole
 * (font, block) tasks per lane, manager.rs:86-97's unit, and the heaviest blocks' glyphs split between lanes until the lanes'
 * estimated raster cost is within 4 % of the mean; 1 whole tasks only; 0 glyph-level shards of every font (every block
 * merged afterwards).  Same bytes. */
void vg_manager_set_lane_form(vg_manager *m, int form);
int vg_manager_add_font_with_name(vg_manager *m, const char *name, const char *const *paths, int n_paths);
int vg_manager_add_font_data(vg_manager *m, const char *name, const uint8_t *data, size_t len);
/*
 * A VARIABLE file at a position of its design space, under a name of the caller's ("this file, at this position, under this
 * name"): axis_tags[i] (4 bytes, e.g. "wght") is set to values[i] in user space; axes not named stay at their default.  The
 * values are normalised in f32 (clamped to the axis, (v - def) / (def - min) or / (max - def), times 16384, truncated) and sent
 * through the file's `avar` (version 1.0).  CFF2 outlines are drawn at the position, `glyf` outlines are moved by `gvar` (tuple
 * scalars, deltas, inferred points, component offsets: the rules G1 to G6 of csrc/host/ttf_face.hpp) and advances follow `HVAR`
 * (without `HVAR` the `hmtx` advance stands, or, for a `glyf` face placed after vg_manager_set_gvar_advances(m, 1), the
 * advance follows gvar's phantom points: rule G7 there).  A placed `glyf` face is a command
 * face for every form: vg_manager_record_glyf_parts, _resident_font_desc and _font_tables_desc refuse it.  Everything that
 * describes the file afterwards (vg_manager_charstring2_font_desc, _command_font_desc, _family_desc ...) describes it there.
 * Several instances of one file under different names are several font ids; the same name merges them into one font id like
 * any other files; no two instances share a store on a device.  Returns what vg_manager_add_font_data returns; -1 with
 * vg_last_error also for an unknown tag, a tag given twice, a value that is not finite, a file without a readable `fvar`, a
 * face with `glyf` outlines and no readable `gvar` (version 1.0, axisCount equal to fvar's, header, shared tuples and offset array
 * inside the table), an HVAR store of another format than 1 or with 32-bit deltas.  A file added
 * any other way (vg_manager_add_font_data, _add_path, _scan) is at its default position, as the reference renders it.
 * _normalized: the final normalised coordinates (F2Dot14), one per `fvar` axis (at most 64 are counted; another number: -1);
 * nothing is normalised and `avar` is not applied.
 */
int vg_manager_add_font_instance(vg_manager *m, const char *name, const uint8_t *data, size_t len, const char *const *axis_tags,
                                 const float *values, int n);
int vg_manager_add_font_instance_normalized(vg_manager *m, const char *name, const uint8_t *data, size_t len, const int16_t *coords, int n);
/*
 * EVERY NAMED INSTANCE of a variable file as a font id of its own — "Noto Sans Thin ... Black" from one file with one call.  Each
 * instance record of the file's `fvar` is added by the rules of vg_manager_add_font_instance at the record's coordinates (same
 * normalisation, same `avar` handling, same refusals); all instances share ONE copy of the bytes.  CFF2 files are accepted: their
 * instances are drawn at their positions, one store each.  The font id of an instance is parse_font_name(family, ps_name) sent
 * through the name generation every file's id comes from (vg_manager_generate_name, vg_name_to_id), where family is the file's name id 1
 * and ps_name is
 *   - the string of the record's postScriptNameID, when the record carries one that is not 0xFFFF and `name` has it;
 *   - otherwise the variations PostScript name prefix (name id 25) — absent or empty: the family name with everything but ASCII
 *     letters and digits removed —, then "-", then the string of the record's subfamilyNameID with its spaces removed (an id
 *     that `name` does not have: nothing).
 * Two instances that arrive at the same id merge like any files of one id (first provider wins).  Returns the number of
 * instances added and writes the first `cap` font ids (NUL terminated, cut at VG_FONT_ID_MAX - 1 bytes) in the table's order;
 * -1 with vg_last_error, nothing added: no readable `fvar`, no instance record, a face with `glyf` outlines and no readable
 * `gvar`, or anything else vg_manager_add_font_instance refuses.
 * vg_manager_set_scan_named_instances, 0 (default) / 1: vg_manager_scan and vg_manager_add_path treat a variable file that has
 * instance records this way; with 0, and for every other file, they add the file at its default position as the reference does.
 */
#define VG_FONT_ID_MAX 256
int vg_manager_add_font_named_instances(vg_manager *m, const uint8_t *data, size_t len, char (*ids)[VG_FONT_ID_MAX], int cap);
void vg_manager_set_scan_named_instances(vg_manager *m, int on);
/* inspection: the font ids of the faces that share their bytes with the ONE file of font_id — every instance record's id of the
 * file vg_manager_add_font_named_instances took, in the table's order (an id two records arrive at: twice); the first `cap` into
 * ids.  Returns their number; 0 for an unknown id, an id of several files or a file added any other way; negative: an error. */
int vg_manager_instance_group(const vg_manager *m, const char *font_id, char (*ids)[VG_FONT_ID_MAX], int cap);
/* What a file's `fvar` offers (host only), so that a caller can turn "the named instances of this file" into calls of
 * vg_manager_add_font_instance without a font parser of its own.  _axes: the number of axes, and the first `cap` of them in
 * tags / min / def / max (user space; each array may be NULL).  _named_instances: the number of instance records, and the first
 * cap_instances of them in name_id (the subfamily name's id in `name`) and coords [cap_instances * n_axes] (user space); n_axes
 * must be the file's.  -1: no readable `fvar`, or n_axes is not the number of its axes. */
/* test / inspection of a file the manager holds.  _font_position: the number of normalised coordinates file `file_index` of the
 * font id was placed at (0: it was not added at a position), and the first `cap` of them in coords (may be NULL).
 * _font_hor_advances: the file's numGlyphs, and in advances[0 .. cap) the reader's advance of every glyph id in font units
 * (hmtx, plus HVAR — or, for a face that follows G7, gvar's phantom points — for a file at a position; 0 for "none" and for ids
 * at and past numGlyphs).  -1: unknown font / file.
 * _font_gvar_advance_deltas: rule G7 for every glyph id of a `glyf` face placed by `gvar`, WHETHER OR NOT its advances follow it
 * (the switch and an HVAR are not looked at): the file's numGlyphs, and for ids 0 .. cap - 1 the f32 d = r - l in delta[] and
 * in state[] 0 (no variation data, d = 0), 1 (delta) or 2 (malformed: d = 0, hmtx stands) — what vgsdf_gvar_advance_deltas
 * is held to, bit for bit.  -1 as well: not a face placed by gvar. */
int vg_manager_font_position(const vg_manager *m, const char *font_id, int file_index, int16_t *coords, int cap);
int vg_manager_font_hor_advances(const vg_manager *m, const char *font_id, int file_index, uint16_t *advances, int cap);
int vg_manager_font_gvar_advance_deltas(const vg_manager *m, const char *font_id, int file_index, float *delta, uint8_t *state, int cap);
int vg_font_variation_axes(const uint8_t *data, size_t len, char (*tags)[4], float *min, float *def, float *max, int cap);
int vg_font_named_instances(const uint8_t *data, size_t len, uint16_t *name_id, float *coords, int cap_instances, int n_axes);
/* manager.rs:39-53: the file's name table decides the font id (family/width/weight/style ->
 * generate_name -> name_to_id); files with the same id merge in call order. */
int vg_manager_add_path(vg_manager *m, const char *path);
/* recurse.rs:104-133 `scan`: *.ttf / *.otf files are added by add_path; a directory holding a
 * fonts.json ([{name, sources[]}], paths relative to it) is read through that file; other
 * directories are walked, entries in ascending byte order of their names (canonical order). */
int vg_manager_scan(vg_manager *m, const char *path);
/* font ids (ascending), '\n' separated, NUL terminated; returns the needed size incl. NUL */
long vg_manager_font_ids(const vg_manager *m, char *out, size_t cap);
/* raw family names (name id 1) of the files of one font id in wrapper order, '\n' separated */
long vg_manager_font_file_names(const vg_manager *m, const char *font_id, char *out, size_t cap);
/* parse_font_name(family, ps_name): style_out / width_out need 16 bytes each; returns the
 * length of the family (written NUL terminated into family_out, truncated to cap). */
int vg_parse_font_name(const char *family, const char *ps_name, char *family_out, size_t cap, char *style_out,
                       uint16_t *weight_out, char *width_out);
/* FontMetadata::generate_name of file `file_index` of a font id -> out; returns the needed size */
long vg_manager_generate_name(const vg_manager *m, const char *font_id, int file_index, char *out, size_t cap);
/* encode_codeblocks (index_files.rs:65-103); returns the needed size incl. NUL */
long vg_encode_codeblocks(const uint32_t *codepoints, size_t n, char *out, size_t cap);
/* build_index_json / build_font_families_json: returns the needed size (no NUL) */
long vg_manager_index_json(const vg_manager *m, uint8_t *out, size_t cap);
long vg_manager_families_json(const vg_manager *m, uint8_t *out, size_t cap);
/* name_to_id (manager.rs:141-147); writes a NUL-terminated id, returns its length */
int vg_name_to_id(const char *name, char *out, size_t cap);
/* number of code points (<= 0xFFFF) the font id maps after first-provider-wins merging */
int vg_manager_block_counts(const vg_manager *m, const char *font_id, uint32_t counts[256]);
/*
 * Supplementary planes (default off): code points above U+FFFF, which the reference skips (wrapper.rs:66-68).  With the switch
 * on every font id's block table keeps its 256 blocks of the BMP, all of them, empty ones included, and lists behind them one
 * block per POPULATED range [256 b, 256 b + 255] above U+FFFF, ascending, first provider wins as in the BMP; empty supplementary
 * blocks are not written.  vg_manager_render_glyphs writes "<start>-<start + 255>.pbf" for them like any other block;
 * vg_manager_render_blocks and vg_manager_render_block find such a block by its start, and a supplementary start the font id
 * does not populate is "bad block start".  A supplementary block is never split: under vg_manager_set_glyph_shard it belongs
 * whole to rank (start / 256) % world and the other ranks neither list nor write it (vg_manager_render_blocks passes such a
 * start over), so the files of all ranks together are the single-rank files; in a multi-device run it goes whole to that lane.
 * owner[65536] / cost[65536] of vg_manager_shard_glyphs and vg_manager_plan_lanes keep their size and meaning.  The forms that
 * name glyphs (host tessellation, packed, glyf parts, resident fonts and command stores, mixed) take such a block as any other;
 * the ranges forms (vg_manager_set_resident_families) name ONE FAMILY PER PLANE of the font id — same stores, budget and lifetime,
 * each table with a serial of its own — and emit tasks with the low halves; with vg_manager_set_family_tables_on_device a static
 * font id's supplementary families are built by the device, the planes chosen by one census call (vg_family_plane_stats below),
 * otherwise and for a font id with a placed face the host states them from its block table (vgsdf_family_create_at).
 * Union outlines, in-place PBF and VG_MODE_DUMMY work on such a block as on any other.  With the switch off every byte stays what
 * it is.  vg_manager_supplementary_blocks: how many such blocks the font id has (0 with the switch off); fills up to `cap` of
 * starts / counts (each may be NULL), ascending; -1: unknown font id.  vg_manager_block_counts is unchanged.
 */
int vg_manager_set_supplementary_planes(vg_manager *m, int on);
int vg_manager_supplementary_blocks(const vg_manager *m, const char *font_id, uint32_t *starts, uint32_t *counts, int cap);

/* Native sinks (src/writer): a ustar stream into a file or an open descriptor (e.g. 1 = stdout,
 * `recurse --tar`), or a directory tree.  mtime < 0 stamps every tar header with the wall clock as
 * the reference does (tar.rs:68-72); tests pass a fixed time to get reproducible bytes. */
typedef struct vg_writer vg_writer;
vg_writer *vg_writer_new_tar_path(const char *path, int64_t mtime);
vg_writer *vg_writer_new_tar_fd(int fd, int64_t mtime); /* the descriptor is NOT closed */
vg_writer *vg_writer_new_dir(const char *folder);
int vg_writer_write_file(vg_writer *w, const char *path, const uint8_t *data, size_t len);
int vg_writer_write_directory(vg_writer *w, const char *path);
int vg_writer_finish(vg_writer *w); /* idempotent (writer/mod.rs:71-77) */
void vg_writer_free(vg_writer *w);  /* finishes first, like Drop (mod.rs:84-96) */

int vg_manager_render_glyphs(vg_manager *m, vg_renderer *r, vg_write_cb cb, void *user);
/* the same into a native sink; index.json / font_families.json as manager.rs:128-138 */
int vg_manager_render_glyphs_to(vg_manager *m, vg_renderer *r, vg_writer *w);
int vg_manager_write_index_json(const vg_manager *m, vg_writer *w);
int vg_manager_write_families_json(const vg_manager *m, vg_writer *w);
/* Glyph-level shard of a font over `world` ranks: longest-processing-time-first on the
 * estimated raster cost w*h*N of every glyph (from its recorded outline: exact point counts of the
 * quadratic flattening, control-box area), identical on every rank.  owner[65536]: rank per code point,
 * 0xFF = unmapped; cost[65536] (may be NULL): the estimates. */
int vg_manager_shard_glyphs(const vg_manager *m, const char *font_id, uint32_t world, uint8_t *owner, double *cost);
/* The lane plan a run on `world` device lanes would use with the present lane form (1 or hybrid), for one font of the
 * manager: owner[65536] = lane per code point (0xFF = unmapped), *n_split_blocks = blocks of this font whose glyphs are
 * split between lanes, *est_max_over_mean = fullest lane / mean lane in the plan's own weights (all fonts of the manager).
 * Host arithmetic only (no device needed); the plan is kept until a font is added.  Any output pointer may be NULL. */
int vg_manager_plan_lanes(vg_manager *m, const char *font_id, uint32_t world, uint8_t *owner, uint32_t *n_split_blocks, double *est_max_over_mean);
/* From now on every render / build_batch / record_outlines call of this manager sees only the glyphs
 * that rank `rank` of `world` owns; every block is still emitted and its PBF holds this rank's glyphs
 * only (a partial).  world <= 1 switches sharding off. */
int vg_manager_set_glyph_shard(vg_manager *m, uint32_t rank, uint32_t world); /* -1: rank >= world or world > 254 */
/* Merges partial PBFs of ONE block (disjoint glyph subsets, same name and range) into the block's PBF:
 * glyphs in ascending id, byte for byte what a single process encodes.  Returns the needed size. */
long vg_pbf_merge(const uint8_t *const *parts, const size_t *lens, int n, uint8_t *out, size_t cap);
/* the same for parts that hold CONSECUTIVE runs of the block's code points, given in order (the split blocks of the hybrid
 * lane plan): header + the parts' entries as they are, no walk over the glyph messages; parts that are not in that form
 * are handed to vg_pbf_merge's code */
long vg_pbf_concat(const uint8_t *const *parts, const size_t *lens, int n, uint8_t *out, size_t cap);
/* A rank's shard: only the listed block starts (multiples of 256) of one font id. */
int vg_manager_render_blocks(vg_manager *m, vg_renderer *r, const char *font_id, const uint32_t *starts, int n,
                             vg_write_cb cb, void *user);
int vg_manager_timings(const vg_manager *m, vg_timings *out);
/* {blocks, glyphs, pixels} of the last render with a multi-device renderer, as reduced over its lanes (zeros otherwise) */
void vg_manager_reduced_counters(const vg_manager *m, uint64_t counters[3]);
/* GlyphBlock::render for one block of one font -> PBF bytes; returns needed size */
long vg_manager_render_block(vg_manager *m, vg_renderer *r, const char *font_id, uint32_t start, uint8_t *out,
                             size_t cap);

/* Renderer::render_glyph(face, index): 1 = Some, 0 = None.  file_index selects the file
 * inside the font id (wrapper.files order). */
int vg_render_glyph(vg_renderer *r, const vg_manager *m, const char *font_id, int file_index, uint32_t index,
                    vg_pbf_glyph *out, uint8_t *bitmap, size_t cap);

/* Host stage only (cmap -> outline -> flatten -> scale/shift -> bbox) for every glyph of a
 * font id: the SoA batch to hand to vgsdf_batch_upload.  Pointers in *view stay valid
 * until vg_glyph_batch_free.  ids[i] = code point of rasterised glyph i. */
vg_glyph_batch *vg_manager_build_batch(vg_manager *m, const char *font_id);
int vg_glyph_batch_view(const vg_glyph_batch *b, vgsdf_batch *view, const uint32_t **ids, uint32_t *n_jobs);
void vg_glyph_batch_free(vg_glyph_batch *b);

/* Host half of the DEVICE front-end for every glyph of a font id: the recorded outline
 * commands + scale / shift per glyph, i.e. the argument of vgsdf_outlines_prepare.  ids[i] /
 * advances[i] = code point / PBF advance of glyph i.  Valid until vg_outline_batch_free. */
typedef struct vg_outline_batch vg_outline_batch;
vg_outline_batch *vg_manager_record_outlines(const vg_manager *m, const char *font_id);
int vg_outline_batch_view(const vg_outline_batch *b, vgsdf_outlines *view, const uint32_t **ids, const uint32_t **advances);
void vg_outline_batch_free(vg_outline_batch *b);
/* The same for the device's glyf decoder (fonts whose glyphs all have `glyf` outlines; NULL otherwise): nothing is decoded
 * on the host, every glyph's simple glyphs are listed as parts with their arrays copied as they stand — the argument of
 * vgsdf_outlines_submit_glyf (pbf_pre / pbf_fix NULL).  Valid until vg_glyf_batch_free. */
typedef struct vg_glyf_batch vg_glyf_batch;
vg_glyf_batch *vg_manager_record_glyf_parts(const vg_manager *m, const char *font_id);
int vg_glyf_batch_view(const vg_glyf_batch *b, vgsdf_outlines_glyf *view, const uint32_t **ids, const uint32_t **advances);
void vg_glyf_batch_free(vg_glyf_batch *b);

/* Host halves of the resident-font form (vgsdf_font_create / vgsdf_outlines_submit_resident), no device needed.
 * vg_manager_resident_font_desc: the description of file `file_index` of a font id (wrapper.files order) — the leaves of
 * EVERY glyph id of the face, listed by the walk and the checks that record the parts above, every simple glyph's arrays
 * stored once.  Built on first use, kept with the face: the pointers in *desc stay valid as long as the manager holds the
 * font.  -1: unknown font / file, a face without `glyf` outlines, or a face past the bounds of the form (more than 2^22
 * leaves, a glyph of more than 2^26 command slots, a store past what 32-bit offsets address).
 * vg_manager_record_resident: what a submission of every glyph of the font id names — per glyph the file (font_of, an index
 * into the font id's files) and the glyph id, scale / shift_x, and ids[i] / advances[i] as above.  NULL when a file of the
 * font has no resident form.  Valid until vg_resident_batch_free. */
typedef struct vg_resident_batch vg_resident_batch;
typedef struct {
	uint32_t n_glyphs, n_files;
	const uint16_t *font_of;  /* [n_glyphs] */
	const uint16_t *glyph_id; /* [n_glyphs] */
	const double *scale;      /* [n_glyphs] */
	const double *shift_x;    /* [n_glyphs] */
	const uint32_t *ids;      /* [n_glyphs] code points */
	const uint32_t *advances; /* [n_glyphs] */
} vg_resident_view;
int vg_manager_resident_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_desc *desc);
vg_resident_batch *vg_manager_record_resident(const vg_manager *m, const char *font_id);
int vg_resident_batch_view(const vg_resident_batch *b, vg_resident_view *view);
void vg_resident_batch_free(vg_resident_batch *b);
/* The same against command fonts (vgsdf_font_create_commands), for EVERY face the reader can read — CFF and CFF2 charstrings,
 * `glyf` faces the forms above refuse — no device needed.
 * vg_manager_command_font_desc: for every glyph id of file `file_index` the callbacks the reader delivers for it, in the arrays
 * of the packed form: exactly what a render of the glyph records today (a glyph whose charstring or entry fails midway holds
 * the callbacks delivered up to there).  Built on first use, kept with the face; the pointers stay valid as long as the manager
 * holds the font.  -1: unknown font / file, or a face whose store on the device (29 bytes per command, 4 per glyph id) or whose coordinates
 * would pass what 32-bit offsets address (refused by counting the callbacks, before the table is allocated).
 * vg_manager_record_resident_commands: what a submission of every glyph of the font id names, as vg_manager_record_resident
 * (the same view, freed the same way); NULL for an unknown font id or a file without a command table. */
int vg_manager_command_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_cmds_desc *desc);
/* The description of file `file_index` for vgsdf_font_create_charstrings, without a device: the face's charstrings and
 * subroutine bodies and their resolved INDEX offsets, built once per face; no charstring is interpreted.  The pointers stay valid
 * as long as the manager holds the font.  -1: unknown font / file, a face with `glyf` outlines, a CFF2 face, or a `CFF ` table whose
 * INDEX entries do not ascend inside their data. */
int vg_manager_charstring_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_charstrings_desc *desc);
/* The same of a CFF2 face for vgsdf_font_create_charstrings2: INDEX counts read as 32 bits, the one set of local subroutines the
 * reader uses for every glyph, and the blend sets — one per ItemVariationData of the variation store, with its usable flag and the
 * factors the reader multiplies `blend` deltas by (at the file's position: the default one unless it is an instance).  -1: unknown font / file, anything that is not CFF2, an
 * INDEX whose entries do not ascend inside their data, or a set of more than 65535 subroutines. */
int vg_manager_charstring2_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_charstrings2_desc *desc);
/* The batched description (vgsdf_fonts_create_charstrings2) of the instance group the ONE file of font_id belongs to —
 * vg_manager_instance_group's, in its order: position p's slice of face.factors is what vg_manager_charstring2_font_desc gives
 * for instance p, everything else is the first face's.  Views that stay valid while the manager holds the fonts.  -1: where
 * vg_manager_charstring2_font_desc(m, font_id, 0, ...) returns -1, a font id that is not in a group, or faces of the group that
 * disagree in anything but the factors (one file, one parse: they cannot). */
int vg_manager_charstring2_fonts_desc(const vg_manager *m, const char *font_id, vgsdf_fonts_charstrings2_desc *desc);
vg_resident_batch *vg_manager_record_resident_commands(const vg_manager *m, const char *font_id);

/* The host half of a resident family (vgsdf_family_create / vgsdf_outlines_submit_ranges), no device needed: for every code
 * point the font id maps (up to 0xFFFF, strictly ascending) the file that draws it (font_of: an index into the font id's files,
 * first provider wins), its glyph id there, PbfGlyph.advance, scale and shift_x — element for element the arrays of
 * vg_manager_record_resident / _record_resident_commands, whichever kind of store the files get: with fonts[k] the device font
 * of file k, the view is a vgsdf_family_desc.  Built on first use, kept with the manager and rebuilt when a file is added to the
 * font id: the pointers stay valid until then.  -1: unknown font id. */
typedef struct {
	uint32_t n_entries, n_files;
	const uint16_t *code_point; /* [n_entries] */
	const uint16_t *font_of;    /* [n_entries] */
	const uint16_t *glyph_id;   /* [n_entries] */
	const uint32_t *advance;    /* [n_entries] */
	const double *scale;        /* [n_entries] */
	const double *shift_x;      /* [n_entries] */
} vg_family_view;
int vg_manager_family_desc(const vg_manager *m, const char *font_id, vg_family_view *view);
/* The same family stated by its faces' TABLES, for vgsdf_family_create_tables (no device needed, and no code point looked up):
 * file `file_index`'s whole `cmap` and `hmtx` tables as views into the face, units_per_em, num_glyphs (maxp), num_hmetrics (hhea),
 * and the encoding records, in the table's order, that are unicode and of format 0, 4, 6, 10, 12 or 13.  With fonts[k] the device
 * font of file k and tables[k] this description, the device builds the table vg_manager_family_desc states.  The pointers stay
 * valid as long as the manager holds the font.  -1: unknown font / file, or a description that REFUSES: a format 4 subtable whose
 * segments are not regular (segCountX2 >= 2, the arrays inside the table, start <= end, start above the previous end), or a
 * format 12 / 13 subtable whose groups are not ascending and disjoint inside the table, or (a file at a position) an HVAR that
 * vg_manager_family_variation_desc refuses; vg_last_error then begins "refused" and names which. */
int vg_manager_family_tables_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_face_tables *desc);
/* ... and what vgsdf_family_create_tables_var takes beside it for a file at a position (vg_manager_add_font_instance): its whole
 * `HVAR` table as a view into the face, where its store and advance map are, and the factor of every region of the store at the
 * file's position.  A file that is not at a position, or has no readable HVAR: 0 with hvar NULL (a static face).  -1: as above,
 * or an HVAR the description REFUSES — an advance map of a format other than 0 and 1 or outside the table, an ItemVariationData
 * with more word deltas than regions — whose font id gets its family the host's way. */
int vg_manager_family_variation_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_face_variation *desc);
/* A `glyf` face stated by its TABLES, for vgsdf_font_create_tables (no device needed, and no glyph looked at): file `file_index`'s
 * whole `loca` and `glyf` tables as views into the face, num_glyphs (maxp), the loca format (head) and the loca entries the reader
 * goes by.  The device builds from it the leaves vg_manager_resident_font_desc states, with the simple entries' bytes in glyph-id
 * order.  The pointers stay valid as long as the manager holds the font.  -1: unknown font / file, or a face without `glyf`
 * outlines (vg_last_error then begins "refused"). */
int vg_manager_font_tables_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_tables_desc *desc);
/* The same of a `glyf` face placed by `gvar` for vgsdf_font_create_gvar: views of its loca, glyf and gvar and of its normalised
 * coordinates, alive as long as the manager holds the file.  -1 for every other face. */
int vg_manager_gvar_font_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_gvar_desc *desc);
/* Beside vg_manager_family_variation_desc: what vgsdf_family_create_tables_gvar takes for file `file_index` of the font id — the
 * description above when the face's advances follow gvar's phantom points (placed with vg_manager_set_gvar_advances on, glyf +
 * gvar, no readable HVAR), all zero (gvar NULL: hand the call a NULL for this face) for every other face.  -1: unknown font /
 * file. */
int vg_manager_family_gvar_desc(const vg_manager *m, const char *font_id, int file_index, vgsdf_font_gvar_desc *desc);

/* Hand-encoder of the glyphs PBF (src/protobuf/glyphs.rs:66-70) for already rendered
 * glyphs; bitmaps[i] may be NULL when !has_bitmap. Returns needed size. */
long vg_pbf_encode(const char *name, const char *range, const vg_pbf_glyph *glyphs, const uint8_t *const *bitmaps,
                   int n, uint8_t *out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
