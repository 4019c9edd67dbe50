"""ctypes binding of include/vgfont.h: FontManager / Renderer / GlyphBlock façade (C++).

Mirrors the reference's names (src/font/manager.rs, src/render/renderer.rs) so tests read
like the reference's own tests.  HIP mode has no CPU fallback; Renderer.new_precise()
raises when no MI355X/HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from .device import OUTLINE_CMD_DTYPE, Batch, VgsdfError, _CBatch, _COutlines, load_library

MODE_HIP, MODE_DUMMY = 0, 1


class PbfGlyph(C.Structure):
    _fields_ = [("id", C.c_uint32), ("has_bitmap", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("left", C.c_int32), ("top", C.c_int32), ("advance", C.c_uint32), ("bitmap_len", C.c_uint32)]
    bitmap = None  # numpy u8 [height+6, width+6] or None

    def metrics(self):
        return (self.width, self.height, self.left, self.top, self.advance)


class Timings(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("tessellate_s", "pack_s", "device_s", "encode_s", "write_s", "total_s")] + \
               [(k, C.c_uint64) for k in ("blocks", "glyphs", "rasters", "pixels", "segments", "pbf_bytes", "glyf_groups", "glyf_fallbacks",
                                                 "fe_groups", "fe_max_group_glyphs")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _CFamilyView(C.Structure):  # vg_family_view
    _fields_ = [("n_entries", C.c_uint32), ("n_files", C.c_uint32), ("code_point", C.c_void_p), ("font_of", C.c_void_p),
                ("glyph_id", C.c_void_p), ("advance", C.c_void_p), ("scale", C.c_void_p), ("shift_x", C.c_void_p)]


class _CResidentView(C.Structure):  # vg_resident_view
    _fields_ = [("n_glyphs", C.c_uint32), ("n_files", C.c_uint32), ("font_of", C.c_void_p), ("glyph_id", C.c_void_p),
                ("scale", C.c_void_p), ("shift_x", C.c_void_p), ("ids", C.c_void_p), ("advances", C.c_void_p)]


class ResidentStats(C.Structure):  # vg_resident_stats
    _fields_ = [(k, C.c_uint64) for k in ("groups", "fonts_uploaded", "font_bytes", "block_bytes")]


class MixedStats(C.Structure):  # vg_mixed_stats
    _fields_ = [(k, C.c_uint64) for k in ("groups", "glyf_fonts", "command_fonts", "block_bytes")]


class _CFaceTables(C.Structure):  # vgsdf_face_tables
    _fields_ = [("cmap", C.c_void_p), ("cmap_len", C.c_uint32), ("hmtx", C.c_void_p), ("hmtx_len", C.c_uint32),
                ("units_per_em", C.c_uint16), ("num_glyphs", C.c_uint16), ("num_hmetrics", C.c_uint16), ("n_subtables", C.c_uint16),
                ("subtable_off", C.c_void_p), ("subtable_format", C.c_void_p)]


class _CFaceVariation(C.Structure):  # vgsdf_face_variation
    _fields_ = [("hvar", C.c_void_p), ("hvar_len", C.c_uint32), ("store_off", C.c_uint32), ("map_off", C.c_uint32),
                ("region_scalars", C.c_void_p), ("n_regions", C.c_uint32)]


class FamilyTableStats(C.Structure):  # vg_family_table_stats
    _fields_ = [(k, C.c_uint64) for k in ("built_on_device", "fallbacks")]


class FamilyPlaneStats(C.Structure):  # vg_family_plane_stats
    _fields_ = [(k, C.c_uint64) for k in ("census_calls", "built_on_device", "stated_by_host", "planes")]


class GlyfTableStats(C.Structure):  # vg_glyf_table_stats
    _fields_ = [(k, C.c_uint64) for k in ("built_on_device", "bytes", "fallbacks")]


class GlyfTableBatchStats(C.Structure):  # vg_glyf_table_batch_stats
    _fields_ = [("calls", C.c_uint64), ("faces", C.c_uint64)]


class FamilyBatchStats(C.Structure):  # vg_family_batch_stats
    _fields_ = [("calls", C.c_uint64), ("families", C.c_uint64)]


class CharstringStats(C.Structure):  # vg_charstring_stats
    _fields_ = [(k, C.c_uint64) for k in ("fonts_decoded", "font_bytes", "fallbacks")]


class GvarStats(C.Structure):  # vg_gvar_stats
    _fields_ = [(k, C.c_uint64) for k in ("fonts_built", "font_bytes", "fallbacks")]


class GvarAdvanceStats(C.Structure):  # vg_gvar_advance_stats
    _fields_ = [(k, C.c_uint64) for k in ("faces", "device_builds", "fallbacks")]


WRITE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_int)

VGFONT_SYMBOLS = [
    "vg_last_error", "vg_renderer_new", "vg_renderer_free", "vg_manager_new", "vg_manager_free",
    "vg_manager_set_threads", "vg_manager_set_device_front_end", "vg_manager_set_union_outlines", "vg_manager_union_stats", "vg_manager_add_font_with_name", "vg_manager_add_font_data", "vg_manager_add_path",
    "vg_manager_set_supplementary_planes", "vg_manager_supplementary_blocks", "vg_manager_family_plane_stats",
    "vg_name_to_id", "vg_manager_block_counts", "vg_manager_render_glyphs", "vg_manager_timings",
    "vg_manager_render_block", "vg_manager_render_blocks", "vg_render_glyph", "vg_manager_build_batch", "vg_glyph_batch_view",
    "vg_glyph_batch_free", "vg_manager_record_outlines", "vg_outline_batch_view", "vg_outline_batch_free", "vg_pbf_encode", "vg_manager_family_desc",
    "vg_manager_record_glyf_parts", "vg_glyf_batch_view", "vg_glyf_batch_free",
    "vg_manager_resident_font_desc", "vg_manager_record_resident", "vg_resident_batch_view", "vg_resident_batch_free",
    "vg_manager_command_font_desc", "vg_manager_record_resident_commands", "vg_manager_set_resident_commands",
    "vg_manager_command_stats", "vg_manager_charstring_font_desc", "vg_manager_charstring2_font_desc", "vg_manager_set_charstrings_on_device",
    "vg_manager_charstring_stats", "vg_manager_charstring_preload_stats", "vg_manager_set_resident_families", "vg_manager_family_stats",
    "vg_manager_set_resident_fonts", "vg_renderer_set_resident_budget", "vg_renderer_preload_fonts", "vg_manager_resident_stats",
    "vg_manager_scan", "vg_manager_font_ids", "vg_manager_font_file_names", "vg_parse_font_name", "vg_manager_generate_name",
    "vg_encode_codeblocks", "vg_manager_index_json", "vg_manager_families_json", "vg_writer_new_tar_path",
    "vg_writer_new_tar_fd", "vg_writer_new_dir", "vg_writer_write_file", "vg_writer_write_directory", "vg_writer_finish",
    "vg_writer_free", "vg_manager_render_glyphs_to", "vg_manager_write_index_json", "vg_manager_write_families_json",
    "vg_manager_shard_glyphs", "vg_manager_set_glyph_shard", "vg_pbf_merge", "vg_pbf_concat",
    "vg_renderer_new_multi", "vg_renderer_device_count", "vg_renderer_reduce_counters", "vg_renderer_reduce_path", "vg_renderer_add_counters",
    "vg_renderer_reset_counters", "vg_manager_reduced_counters", "vg_manager_set_in_place_pbf", "vg_manager_set_glyf_on_device", "vg_manager_set_lane_form", "vg_manager_plan_lanes",
    "vg_manager_family_tables_desc", "vg_manager_font_tables_desc", "vg_manager_set_family_tables_on_device", "vg_manager_family_table_stats",
    "vg_manager_set_glyf_tables_on_device", "vg_manager_glyf_table_stats",
    "vg_manager_set_gvar_on_device", "vg_manager_gvar_stats", "vg_manager_gvar_font_desc",
    "vg_manager_set_glyf_tables_batched", "vg_manager_glyf_table_batch_stats",
    "vg_manager_set_mixed_stores", "vg_manager_mixed_stats",
    "vg_manager_add_font_instance", "vg_manager_add_font_instance_normalized", "vg_font_variation_axes", "vg_font_named_instances",
    "vg_manager_family_variation_desc", "vg_manager_font_position", "vg_manager_font_hor_advances",
    "vg_manager_add_font_named_instances", "vg_manager_set_scan_named_instances", "vg_manager_set_gvar_batched", "vg_manager_gvar_batch_stats",
    "vg_manager_set_charstrings_batched", "vg_manager_charstring_batch_stats", "vg_manager_charstring2_fonts_desc",
    "vg_manager_set_family_tables_batched", "vg_manager_family_batch_stats", "vg_manager_instance_group",
    "vg_manager_set_gvar_advances", "vg_manager_gvar_advance_stats", "vg_manager_font_gvar_advance_deltas",
    "vg_manager_family_gvar_desc",
]

VG_FONT_ID_MAX = 256

_bound = False


def _L():
    global _bound
    L = load_library()
    if not _bound:
        vp = C.c_void_p
        L.vg_last_error.restype = C.c_char_p
        L.vg_renderer_new.restype = vp
        L.vg_renderer_new.argtypes = [C.c_int, C.c_int]
        L.vg_renderer_free.argtypes = [vp]
        L.vg_manager_new.restype = vp
        L.vg_manager_new.argtypes = [C.c_int]
        L.vg_manager_free.argtypes = [vp]
        L.vg_manager_set_threads.argtypes = [vp, C.c_uint, C.c_uint]
        L.vg_manager_set_device_front_end.argtypes = [vp, C.c_int]
        L.vg_manager_set_device_front_end.restype = None
        L.vg_manager_set_union_outlines.argtypes = [vp, C.c_int]
        L.vg_manager_set_union_outlines.restype = None
        L.vg_manager_union_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
        L.vg_manager_union_stats.restype = None
        L.vg_manager_set_in_place_pbf.argtypes = [vp, C.c_int]
        L.vg_manager_set_in_place_pbf.restype = None
        L.vg_manager_set_glyf_on_device.argtypes = [vp, C.c_int]
        L.vg_manager_set_glyf_on_device.restype = None
        L.vg_manager_set_resident_fonts.argtypes = [vp, C.c_int]
        L.vg_manager_set_resident_fonts.restype = None
        L.vg_renderer_set_resident_budget.argtypes = [vp, C.c_uint64]
        L.vg_renderer_set_resident_budget.restype = None
        L.vg_renderer_preload_fonts.argtypes = [vp, vp]
        L.vg_renderer_preload_fonts.restype = C.c_longlong
        L.vg_manager_resident_stats.argtypes = [vp, C.POINTER(ResidentStats)]
        L.vg_manager_set_resident_commands.argtypes = [vp, C.c_int]
        L.vg_manager_set_resident_commands.restype = None
        L.vg_manager_command_stats.argtypes = [vp, C.POINTER(ResidentStats)]
        L.vg_manager_set_mixed_stores.argtypes = [vp, C.c_int]
        L.vg_manager_set_mixed_stores.restype = None
        L.vg_manager_mixed_stats.argtypes = [vp, C.POINTER(MixedStats)]
        L.vg_manager_set_charstrings_on_device.argtypes = [vp, C.c_int]
        L.vg_manager_set_charstrings_on_device.restype = None
        L.vg_manager_charstring_stats.argtypes = [vp, C.POINTER(CharstringStats)]
        L.vg_manager_charstring_preload_stats.argtypes = [vp, C.POINTER(CharstringStats)]
        L.vg_manager_set_resident_families.argtypes = [vp, C.c_int]
        L.vg_manager_set_resident_families.restype = None
        L.vg_manager_family_stats.argtypes = [vp, C.POINTER(ResidentStats)]
        L.vg_manager_family_desc.argtypes = [vp, C.c_char_p, vp]
        L.vg_manager_family_tables_desc.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(_CFaceTables)]
        L.vg_manager_set_family_tables_on_device.argtypes = [vp, C.c_int]
        L.vg_manager_set_family_tables_on_device.restype = None
        L.vg_manager_family_table_stats.argtypes = [vp, C.POINTER(FamilyTableStats)]
        L.vg_manager_family_plane_stats.argtypes = [vp, C.POINTER(FamilyPlaneStats)]
        L.vg_manager_set_glyf_tables_on_device.argtypes = [vp, C.c_int]
        L.vg_manager_set_glyf_tables_on_device.restype = None
        L.vg_manager_set_gvar_on_device.argtypes = [vp, C.c_int]
        L.vg_manager_set_gvar_on_device.restype = None
        L.vg_manager_gvar_stats.argtypes = [vp, C.POINTER(GvarStats)]
        L.vg_manager_glyf_table_stats.argtypes = [vp, C.POINTER(GlyfTableStats)]
        L.vg_manager_set_glyf_tables_batched.argtypes = [vp, C.c_int]
        L.vg_manager_set_glyf_tables_batched.restype = None
        L.vg_manager_glyf_table_batch_stats.argtypes = [vp, C.POINTER(GlyfTableBatchStats)]
        L.vg_manager_add_font_named_instances.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_int]
        L.vg_manager_set_scan_named_instances.argtypes = [vp, C.c_int]
        L.vg_manager_set_scan_named_instances.restype = None
        L.vg_manager_set_gvar_batched.argtypes = [vp, C.c_int]
        L.vg_manager_set_gvar_batched.restype = None
        L.vg_manager_gvar_batch_stats.argtypes = [vp, C.POINTER(GlyfTableBatchStats)]
        L.vg_manager_set_charstrings_batched.argtypes = [vp, C.c_int]
        L.vg_manager_set_charstrings_batched.restype = None
        L.vg_manager_charstring_batch_stats.argtypes = [vp, C.POINTER(GlyfTableBatchStats)]
        L.vg_manager_charstring2_fonts_desc.argtypes = [vp, C.c_char_p, C.c_void_p]
        L.vg_manager_set_family_tables_batched.argtypes = [vp, C.c_int]
        L.vg_manager_set_family_tables_batched.restype = None
        L.vg_manager_family_batch_stats.argtypes = [vp, C.POINTER(FamilyBatchStats)]
        L.vg_manager_instance_group.argtypes = [vp, C.c_char_p, vp, C.c_int]
        L.vg_manager_set_lane_form.argtypes = [vp, C.c_int]
        L.vg_manager_set_lane_form.restype = None
        L.vg_manager_plan_lanes.argtypes = [vp, C.c_char_p, C.c_uint32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        L.vg_manager_add_font_with_name.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), C.c_int]
        L.vg_manager_add_font_data.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
        L.vg_manager_add_path.argtypes = [vp, C.c_char_p]
        L.vg_manager_add_font_instance.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
        L.vg_manager_add_font_instance_normalized.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int16), C.c_int]
        L.vg_font_variation_axes.argtypes = [C.c_char_p, C.c_size_t, vp, vp, vp, vp, C.c_int]
        L.vg_font_named_instances.argtypes = [C.c_char_p, C.c_size_t, vp, vp, C.c_int, C.c_int]
        L.vg_manager_family_variation_desc.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(_CFaceVariation)]
        L.vg_manager_font_position.argtypes = [vp, C.c_char_p, C.c_int, vp, C.c_int]
        L.vg_manager_font_hor_advances.argtypes = [vp, C.c_char_p, C.c_int, vp, C.c_int]
        L.vg_manager_font_gvar_advance_deltas.argtypes = [vp, C.c_char_p, C.c_int, vp, vp, C.c_int]
        L.vg_manager_set_gvar_advances.argtypes = [vp, C.c_int]
        L.vg_manager_set_gvar_advances.restype = None
        L.vg_manager_gvar_advance_stats.argtypes = [vp, C.POINTER(GvarAdvanceStats)]
        L.vg_name_to_id.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        L.vg_manager_block_counts.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32)]
        L.vg_manager_set_supplementary_planes.argtypes = [vp, C.c_int]
        L.vg_manager_supplementary_blocks.argtypes = [vp, C.c_char_p, vp, vp, C.c_int]
        L.vg_manager_render_glyphs.argtypes = [vp, vp, WRITE_CB, vp]
        L.vg_manager_render_blocks.argtypes = [vp, vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_int, WRITE_CB, vp]
        L.vg_manager_timings.argtypes = [vp, C.POINTER(Timings)]
        L.vg_manager_render_block.restype = C.c_long
        L.vg_manager_render_block.argtypes = [vp, vp, C.c_char_p, C.c_uint32, vp, C.c_size_t]
        L.vg_render_glyph.argtypes = [vp, vp, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(PbfGlyph), vp, C.c_size_t]
        L.vg_manager_build_batch.restype = vp
        L.vg_manager_build_batch.argtypes = [vp, C.c_char_p]
        L.vg_glyph_batch_view.argtypes = [vp, C.POINTER(_CBatch), C.POINTER(C.POINTER(C.c_uint32)),
                                          C.POINTER(C.c_uint32)]
        L.vg_glyph_batch_free.argtypes = [vp]
        L.vg_manager_record_outlines.restype = vp
        L.vg_manager_record_outlines.argtypes = [vp, C.c_char_p]
        L.vg_outline_batch_view.argtypes = [vp, C.POINTER(_COutlines), C.POINTER(C.POINTER(C.c_uint32)),
                                            C.POINTER(C.POINTER(C.c_uint32))]
        L.vg_outline_batch_free.argtypes = [vp]
        L.vg_pbf_encode.restype = C.c_long
        L.vg_pbf_encode.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PbfGlyph), C.POINTER(C.c_void_p), C.c_int,
                                    vp, C.c_size_t]
        L.vg_manager_scan.argtypes = [vp, C.c_char_p]
        L.vg_manager_shard_glyphs.argtypes = [vp, C.c_char_p, C.c_uint32, vp, vp]
        L.vg_manager_set_glyph_shard.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.vg_renderer_new_multi.restype = vp
        L.vg_renderer_new_multi.argtypes = [C.POINTER(C.c_int), C.c_int]
        L.vg_renderer_device_count.argtypes = [vp]
        L.vg_renderer_reduce_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.vg_renderer_reduce_path.argtypes = [vp]
        L.vg_renderer_reduce_path.restype = C.c_char_p
        L.vg_renderer_add_counters.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64]
        L.vg_renderer_add_counters.restype = None
        L.vg_renderer_reset_counters.argtypes = [vp]
        L.vg_renderer_reset_counters.restype = None
        L.vg_manager_reduced_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.vg_manager_reduced_counters.restype = None
        L.vg_pbf_merge.restype = C.c_long
        L.vg_pbf_merge.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, vp, C.c_size_t]
        L.vg_pbf_concat.restype = C.c_long
        L.vg_pbf_concat.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, vp, C.c_size_t]
        for f in (L.vg_manager_font_ids, L.vg_manager_index_json, L.vg_manager_families_json):
            f.restype = C.c_long
            f.argtypes = [vp, vp, C.c_size_t]
        L.vg_manager_font_file_names.restype = C.c_long
        L.vg_manager_font_file_names.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
        L.vg_parse_font_name.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_uint16),
                                         C.c_char_p]
        L.vg_manager_generate_name.restype = C.c_long
        L.vg_manager_generate_name.argtypes = [vp, C.c_char_p, C.c_int, vp, C.c_size_t]
        L.vg_encode_codeblocks.restype = C.c_long
        L.vg_encode_codeblocks.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
        L.vg_writer_new_tar_path.restype = vp
        L.vg_writer_new_tar_path.argtypes = [C.c_char_p, C.c_int64]
        L.vg_writer_new_tar_fd.restype = vp
        L.vg_writer_new_tar_fd.argtypes = [C.c_int, C.c_int64]
        L.vg_writer_new_dir.restype = vp
        L.vg_writer_new_dir.argtypes = [C.c_char_p]
        L.vg_writer_write_file.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
        L.vg_writer_write_directory.argtypes = [vp, C.c_char_p]
        L.vg_writer_finish.argtypes = [vp]
        L.vg_writer_free.argtypes = [vp]
        L.vg_writer_free.restype = None
        L.vg_manager_render_glyphs_to.argtypes = [vp, vp, vp]
        L.vg_manager_write_index_json.argtypes = [vp, vp]
        L.vg_manager_write_families_json.argtypes = [vp, vp]
        _bound = True
    return L


def _err() -> str:
    return (_L().vg_last_error() or b"").decode()


def variation_axes(data: bytes):
    """what a file's fvar offers (vg_font_variation_axes): [(tag, min, default, max)] in user space; [] without a readable fvar"""
    L = _L()
    n = L.vg_font_variation_axes(data, len(data), None, None, None, None, 0)
    if n <= 0:
        return []
    tags = (C.c_char * (4 * n))()
    lo, de, hi = ((C.c_float * n)() for _ in range(3))
    L.vg_font_variation_axes(data, len(data), tags, lo, de, hi, n)
    return [(bytes(tags[4 * i:4 * i + 4]).decode("latin-1"), float(lo[i]), float(de[i]), float(hi[i])) for i in range(n)]


def named_instances(data: bytes):
    """the named instances of a file's fvar (vg_font_named_instances): [(subfamily name id, {tag: user-space value})]"""
    L = _L()
    axes = variation_axes(data)
    if not axes:
        return []
    n = L.vg_font_named_instances(data, len(data), None, None, 0, len(axes))
    if n <= 0:
        return []
    ids, co = (C.c_uint16 * n)(), (C.c_float * (n * len(axes)))()
    L.vg_font_named_instances(data, len(data), ids, co, n, len(axes))
    return [(int(ids[k]), {axes[i][0]: float(co[k * len(axes) + i]) for i in range(len(axes))}) for k in range(n)]


def name_to_id(name: str) -> str:
    buf = C.create_string_buffer(1024)
    _L().vg_name_to_id(name.encode(), buf, len(buf))
    return buf.value.decode()


class Renderer:
    """src/render/renderer.rs Renderer; Precise == the HIP back-end."""

    def __init__(self, handle, mode):
        self._h, self.mode = handle, mode

    @classmethod
    def new(cls, dummy: bool, device: int = 0):
        return cls.new_dummy() if dummy else cls.new_precise(device)

    @classmethod
    def new_precise(cls, device: int = 0):
        h = _L().vg_renderer_new(MODE_HIP, device)
        if not h:
            raise VgsdfError(-2, _err())
        return cls(h, MODE_HIP)

    @classmethod
    def new_dummy(cls):
        return cls(_L().vg_renderer_new(MODE_DUMMY, 0), MODE_DUMMY)

    @classmethod
    def new_multi(cls, devices):
        """ONE process, one lane per entry of `devices` (an entry may repeat a device): FontManager.render_glyphs deals a
        font's glyphs to the lanes and merges their partial PBFs in this process (include/vgfont.h)."""
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = _L().vg_renderer_new_multi(devs, len(devices))
        if not h:
            raise VgsdfError(-2, _err())
        return cls(h, MODE_HIP)

    @property
    def n_devices(self) -> int:
        return int(_L().vg_renderer_device_count(self._h))

    def add_counters(self, lane: int, blocks: int, glyphs: int, pixels: int):
        _L().vg_renderer_add_counters(self._h, lane, blocks, glyphs, pixels)

    def reset_counters(self):
        _L().vg_renderer_reset_counters(self._h)

    def set_resident_budget(self, bytes_per_device: int):
        """HBM the device copies of resident fonts may take per device (default 1 GiB; a face that does not fit is rendered
        through the glyf form)"""
        _L().vg_renderer_set_resident_budget(self._h, bytes_per_device)

    def preload_fonts(self, manager) -> int:
        """uploads every face of the manager now -> bytes put on the devices"""
        n = int(_L().vg_renderer_preload_fonts(self._h, manager._h))
        if n < 0:
            raise RuntimeError(_err())
        return n

    def reduce_counters(self):
        """(blocks, glyphs, pixels) summed over the lanes: vgsdf_reduce_counters (RCCL when the devices are distinct)"""
        out = (C.c_uint64 * 3)()
        if _L().vg_renderer_reduce_counters(self._h, out) != 0:
            raise RuntimeError(_err())
        return tuple(int(v) for v in out)

    def reduce_path(self) -> str:
        """how the last reduce took its sum: "rccl", "host: contexts share a device", "host: RCCL fallback: <reason>" ..."""
        return (_L().vg_renderer_reduce_path(self._h) or b"").decode()

    def render_glyph(self, manager: "FontManager", font_id: str, index: int, file_index: int = 0):
        """Renderer::render_glyph(&face, index) -> PbfGlyph | None"""
        g = PbfGlyph()
        buf = np.empty(1 << 20, dtype=np.uint8)
        rc = _L().vg_render_glyph(self._h, manager._h, font_id.encode(), file_index, index, C.byref(g),
                                  buf.ctypes.data, buf.size)
        if rc < 0:
            raise RuntimeError(_err())
        if rc == 0:
            return None
        if g.has_bitmap:
            g.bitmap = buf[:g.bitmap_len].reshape(g.height + 6, g.width + 6).copy()
        return g

    def close(self):
        if self._h:
            _L().vg_renderer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GlyphBatchHost:
    """Owner of a host SoA batch produced by the C++ tessellation stage."""

    def __init__(self, handle):
        self._h = handle
        cb = _CBatch()
        ids = C.POINTER(C.c_uint32)()
        nj = C.c_uint32(0)
        _L().vg_glyph_batch_view(handle, C.byref(cb), C.byref(ids), C.byref(nj))
        n = cb.n_glyphs
        self.n_jobs = nj.value

        def arr(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count)

        seg_off = arr(cb.seg_off, n + 1, np.uint32)
        s = int(seg_off[-1]) if n else 0
        self.batch = Batch(seg_off, arr(cb.seg_sx, s, np.float64), arr(cb.seg_sy, s, np.float64),
                           arr(cb.seg_ex, s, np.float64), arr(cb.seg_ey, s, np.float64), arr(cb.x0, n, np.int32),
                           arr(cb.y0, n, np.int32), arr(cb.w, n, np.uint32), arr(cb.h, n, np.uint32),
                           arr(cb.out_off, n + 1, np.uint64))
        self.ids = arr(C.cast(ids, C.c_void_p).value, n, np.uint32)

    def free(self):
        if self._h:
            _L().vg_glyph_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FontManager:
    """src/font/manager.rs FontManager (render path only)."""

    def __init__(self, parallel: bool = True):
        self._h = _L().vg_manager_new(1 if parallel else 0)
        self._cb_keepalive = None

    def set_threads(self, threads: int = 0, blocks_per_batch: int = 0):
        _L().vg_manager_set_threads(self._h, threads, blocks_per_batch)

    def set_in_place_pbf(self, on: bool):
        """True (default): the raster stores bitmaps where the finished PBF has them; False: blocks are encoded afterwards"""
        _L().vg_manager_set_in_place_pbf(self._h, 1 if on else 0)

    def set_glyf_on_device(self, on: bool):
        """True (default): glyf fonts are decoded on the device; False: the host reader records the outline callbacks"""
        _L().vg_manager_set_glyf_on_device(self._h, 1 if on else 0)

    def set_resident_fonts(self, on: bool):
        """False (default).  True: groups of glyf fonts are submitted by (font, glyph id) against the renderer's device copies of
        the faces (uploaded on first use); same bytes either way"""
        _L().vg_manager_set_resident_fonts(self._h, 1 if on else 0)

    def resident_stats(self) -> dict:
        """of the last render: groups submitted in the resident form, faces uploaded during it, their bytes on the device, bytes
        of the submissions' upload blocks"""
        s = ResidentStats()
        _L().vg_manager_resident_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in ResidentStats._fields_}

    def set_resident_commands(self, mode: int):
        """0 (default).  1: groups that cannot take a glyf form (CFF / CFF2 faces, fonts the device refused) are submitted by
        (font, glyph id) against command stores instead of being read by the host on every render; 2: every group is; same
        bytes in every mode"""
        _L().vg_manager_set_resident_commands(self._h, int(mode))

    def set_mixed_stores(self, on: bool):
        """with the device's glyf decoder, resident fonts and set_resident_commands(1): a group that is not all `glyf` is submitted
        against stores of BOTH kinds, a glyf store for every `glyf` file and a command store for every other, instead of against
        command stores of all its files; same bytes (default off)"""
        _L().vg_manager_set_mixed_stores(self._h, int(bool(on)))

    def mixed_stats(self) -> dict:
        """of the last render: {groups, glyf_fonts, command_fonts, block_bytes} of the groups submitted against stores of both
        kinds (vg_mixed_stats)"""
        s = MixedStats()
        _L().vg_manager_mixed_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in MixedStats._fields_}

    def set_charstrings_on_device(self, on):
        """False / 0 (default).  True / 1: the command stores of `CFF ` version 1 faces are decoded on the device from the charstrings
        (vgsdf_font_create_charstrings) instead of built by the host's reader; a face the device refuses falls back; same bytes.
        2: CFF2 faces as well (vgsdf_font_create_charstrings2, the reader's blend factors: those of the file's position, the default
        one unless add_font_instance put it elsewhere)"""
        _L().vg_manager_set_charstrings_on_device(self._h, int(on))

    def charstring_stats(self) -> dict:
        """of the last render: {fonts_decoded, font_bytes, fallbacks} (vg_charstring_stats)"""
        s = CharstringStats()
        _L().vg_manager_charstring_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in CharstringStats._fields_}

    def charstring_preload_stats(self) -> dict:
        """the same of the manager's last Renderer.preload_fonts (vg_manager_charstring_preload_stats)"""
        s = CharstringStats()
        _L().vg_manager_charstring_preload_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in CharstringStats._fields_}

    def set_resident_families(self, on: bool):
        """groups that would go by (font, glyph id) go as code-point ranges of resident families instead (default off)"""
        _L().vg_manager_set_resident_families(self._h, int(bool(on)))

    def set_family_tables_on_device(self, on: bool):
        """resident families' tables are built by the device from the faces' cmap and hmtx tables (vgsdf_family_create_tables)
        instead of by the host's reader; a font id whose description or build is refused falls back; same bytes (default off)"""
        _L().vg_manager_set_family_tables_on_device(self._h, int(bool(on)))

    def set_gvar_on_device(self, on: bool):
        """the command store of a `glyf` face placed by add_font_instance is built by the DEVICE from loca, glyf and gvar
        (vgsdf_font_create_gvar); a face it refuses goes the host reader's way, once.  Same store and output.  Off by default"""
        _L().vg_manager_set_gvar_on_device(self._h, int(bool(on)))

    def gvar_stats(self) -> dict:
        """of the last render: {fonts_built, font_bytes, fallbacks} (vg_gvar_stats)"""
        s = GvarStats()
        _L().vg_manager_gvar_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in GvarStats._fields_}

    def set_glyf_tables_on_device(self, on: bool):
        """glyf-kind resident fonts are walked by the DEVICE from the faces' loca and glyf tables (vgsdf_font_create_tables): the host
        interprets no glyph.  A face the device refuses falls back to the host's table.  Default off.  Same output"""
        _L().vg_manager_set_glyf_tables_on_device(self._h, int(bool(on)))

    def glyf_table_stats(self) -> dict:
        """of the last render: {built_on_device, bytes, fallbacks} (vg_glyf_table_stats)"""
        s = GlyfTableStats()
        _L().vg_manager_glyf_table_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in GlyfTableStats._fields_}

    def set_glyf_tables_batched(self, on: bool):
        """with set_glyf_tables_on_device: the glyf fonts of all files of a font id are built in ONE call
        (vgsdf_fonts_create_tables) instead of one per file; same fonts, same output (default off)"""
        _L().vg_manager_set_glyf_tables_batched(self._h, int(bool(on)))

    def glyf_table_batch_stats(self) -> dict:
        """of the last render: {calls, faces} of the batched builds (vg_glyf_table_batch_stats)"""
        s = GlyfTableBatchStats()
        _L().vg_manager_glyf_table_batch_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in GlyfTableBatchStats._fields_}

    def family_plane_stats(self) -> dict:
        """of the last render: {census_calls, built_on_device, stated_by_host, planes} (vg_family_plane_stats)"""
        s = FamilyPlaneStats()
        _L().vg_manager_family_plane_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in FamilyPlaneStats._fields_}

    def family_table_stats(self) -> dict:
        """of the last render: {built_on_device, fallbacks} (vg_family_table_stats)"""
        s = FamilyTableStats()
        _L().vg_manager_family_table_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in FamilyTableStats._fields_}

    def family_stats(self) -> dict:
        """of the last render: groups submitted as ranges, families uploaded, their bytes, block bytes (vg_family_stats)"""
        s = ResidentStats()
        _L().vg_manager_family_stats(self._h, C.byref(s))
        return {"groups": int(s.groups), "families_uploaded": int(s.fonts_uploaded), "family_bytes": int(s.font_bytes),
                "block_bytes": int(s.block_bytes)}

    def command_stats(self) -> dict:
        """of the last render: groups submitted by name against command stores, stores uploaded during it, their bytes on the
        device, bytes of those submissions' upload blocks (vg_command_stats: the fields of resident_stats)"""
        s = ResidentStats()
        _L().vg_manager_command_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in ResidentStats._fields_}

    def set_lane_form(self, form: int):
        """several device lanes: -1 / 2 hybrid (whole (font, block) tasks, the heaviest blocks split between lanes), 1 whole tasks
        only, 0 glyph-level shards of every font + merge"""
        _L().vg_manager_set_lane_form(self._h, int(form))

    def set_union_outlines(self, on: bool):
        """union outlines (rule U): the HIP renderer rasters the boundary of every glyph's filled set, so overlapping
        contours leave no seam; the bitmaps are then NOT the reference's.  Off by default; the dummy renderer ignores it"""
        _L().vg_manager_set_union_outlines(self._h, 1 if on else 0)

    def union_stats(self) -> dict:
        """glyphs the union pass saw in this manager's runs: seen = rebuilt + identity + over_limit (+ non-finite)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _L().vg_manager_union_stats(self._h, *[C.byref(x) for x in v])
        return dict(zip(("seen", "rebuilt", "identity", "over_limit"), (int(x.value) for x in v)))

    def set_device_front_end(self, on: bool):
        """flatten / close / scale / bbox on the GPU instead of host threads (HIP renderer only)"""
        _L().vg_manager_set_device_front_end(self._h, 1 if on else 0)

    def add_font_with_name(self, name: str, sources):
        paths = [str(Path(p)).encode() for p in sources]
        arr = (C.c_char_p * len(paths))(*paths)
        if _L().vg_manager_add_font_with_name(self._h, name.encode(), arr, len(paths)) != 0:
            raise RuntimeError(_err())
        return name_to_id(name)

    variation_axes = staticmethod(variation_axes)    # what a file's fvar offers, without a manager
    named_instances = staticmethod(named_instances)

    def add_font_data(self, name: str, data: bytes):
        if _L().vg_manager_add_font_data(self._h, name.encode(), data, len(data)) != 0:
            raise RuntimeError(_err())
        return name_to_id(name)

    def add_font_instance(self, name: str, data: bytes, location: dict):
        """a variable file at a position of its design space under `name` (vg_manager_add_font_instance): location maps axis
        tags to user-space values ({"wght": 650}); axes not named stay at their default"""
        tags = [t.encode() for t in location]
        arr = (C.c_char_p * max(len(tags), 1))(*tags)
        vals = (C.c_float * max(len(tags), 1))(*[float(v) for v in location.values()])
        if _L().vg_manager_add_font_instance(self._h, name.encode(), data, len(data), arr, vals, len(tags)) != 0:
            raise RuntimeError(_err())
        return name_to_id(name)

    def add_font_instance_normalized(self, name: str, data: bytes, coords):
        """the same with final normalised coordinates (F2Dot14 as int16), one per fvar axis; avar is not applied"""
        c = (C.c_int16 * max(len(coords), 1))(*[int(v) for v in coords])
        if _L().vg_manager_add_font_instance_normalized(self._h, name.encode(), data, len(data), c, len(coords)) != 0:
            raise RuntimeError(_err())
        return name_to_id(name)

    def add_font_named_instances(self, data: bytes):
        """vg_manager_add_font_named_instances: every named instance of the file's fvar as a font id of its own, by add_font_instance's
        rules, over ONE copy of the bytes -> the font ids in the table's order (the id rule: include/vgfont.h).  RuntimeError: no
        readable fvar, no instance record, or what add_font_instance refuses"""
        L = _L()
        cap = 4096
        ids = ((C.c_char * VG_FONT_ID_MAX) * cap)()
        n = L.vg_manager_add_font_named_instances(self._h, data, len(data), ids, cap)
        if n < 0:
            raise RuntimeError(_err())
        return [ids[k].value.decode() for k in range(min(n, cap))]

    def set_scan_named_instances(self, on: bool):
        """scan and add_path treat a variable file that has instance records as add_font_named_instances does (default off)"""
        _L().vg_manager_set_scan_named_instances(self._h, int(bool(on)))

    def set_gvar_batched(self, on: bool):
        """with set_gvar_on_device: the command stores of all placed glyf faces over the same bytes (add_font_named_instances) are
        built in ONE call (vgsdf_fonts_create_gvar) instead of one per face; same stores, same output (default off)"""
        _L().vg_manager_set_gvar_batched(self._h, int(bool(on)))

    def gvar_batch_stats(self) -> dict:
        """of the last render: {calls, faces} of the batched gvar builds (vg_gvar_batch_stats)"""
        s = GlyfTableBatchStats()  # (vg_gvar_batch_stats has the same two fields)
        _L().vg_manager_gvar_batch_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in GlyfTableBatchStats._fields_}

    def set_charstrings_batched(self, on: bool):
        """with set_charstrings_on_device(2): the command stores of all placed CFF2 faces over the same bytes
        (add_font_named_instances) are built in ONE call (vgsdf_fonts_create_charstrings2) instead of one per face; same stores,
        same output (default off)"""
        _L().vg_manager_set_charstrings_batched(self._h, int(bool(on)))

    def charstring_batch_stats(self) -> dict:
        """of the last render: {calls, faces} of the batched CFF2 builds (vg_charstring_batch_stats)"""
        s = GlyfTableBatchStats()  # (vg_charstring_batch_stats has the same two fields)
        _L().vg_manager_charstring_batch_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in GlyfTableBatchStats._fields_}

    def set_family_tables_batched(self, on: bool):
        """with set_family_tables_on_device: the family tables of all single-file font ids over the same bytes
        (add_font_named_instances) are built in ONE call (vgsdf_families_create_tables) instead of one per font id; same
        families, same output (default off)"""
        _L().vg_manager_set_family_tables_batched(self._h, int(bool(on)))

    def family_batch_stats(self) -> dict:
        """of the last render: {calls, families} of the batched family-table builds (vg_family_batch_stats)"""
        s = FamilyBatchStats()
        _L().vg_manager_family_batch_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in FamilyBatchStats._fields_}

    def instance_group(self, font_id: str):
        """vg_manager_instance_group: the font ids of the faces that share their bytes with the one file of font_id (every record
        of the file add_font_named_instances took, in the table's order); [] for a static file, a merged id, an unknown id"""
        L = _L()
        cap = 4096
        ids = ((C.c_char * VG_FONT_ID_MAX) * cap)()
        n = L.vg_manager_instance_group(self._h, font_id.encode(), ids, cap)
        if n < 0:
            raise RuntimeError(_err())
        return [ids[k].value.decode() for k in range(min(n, cap))]

    def set_gvar_advances(self, on: bool):
        """vg_manager_set_gvar_advances: glyf + gvar faces placed AFTER the call whose file has no readable HVAR take their
        advances from gvar's phantom points (rule G7 of csrc/host/ttf_face.hpp) instead of keeping hmtx's; not retroactive
        (default off)"""
        _L().vg_manager_set_gvar_advances(self._h, int(bool(on)))

    def gvar_advance_stats(self) -> dict:
        """{faces: placed so far whose advances follow G7; device_builds, fallbacks: of the last render, the families with such a
        face the device built / refused} (vg_gvar_advance_stats)"""
        s = GvarAdvanceStats()
        _L().vg_manager_gvar_advance_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in GvarAdvanceStats._fields_}

    def add_path(self, path):
        """manager.rs:39-53: the file's own name table decides the font id."""
        if _L().vg_manager_add_path(self._h, str(path).encode()) != 0:
            raise RuntimeError(_err())

    def add_paths(self, paths):
        for p in paths:
            self.add_path(p)

    def scan(self, path):
        """recurse.rs:104-133 (fonts.json aware; directory entries in sorted order)."""
        if _L().vg_manager_scan(self._h, str(path).encode()) != 0:
            raise RuntimeError(_err())

    def _text(self, fn, *args) -> bytes:
        need = fn(self._h, *args, None, 0)
        if need < 0:
            raise RuntimeError(_err())
        buf = C.create_string_buffer(need + 1)
        fn(self._h, *args, buf, need + 1)
        return buf.raw[:need]

    def font_ids(self):
        t = self._text(_L().vg_manager_font_ids).rstrip(b"\0").decode()
        return t.split("\n") if t else []

    def font_file_names(self, font_id: str):
        t = self._text(_L().vg_manager_font_file_names, font_id.encode()).rstrip(b"\0").decode()
        return t.split("\n") if t else []

    def generate_name(self, font_id: str, file_index: int = 0) -> str:
        return self._text(_L().vg_manager_generate_name, font_id.encode(), file_index).rstrip(b"\0").decode()

    def index_json(self) -> bytes:
        return self._text(_L().vg_manager_index_json)

    def families_json(self) -> bytes:
        return self._text(_L().vg_manager_families_json)

    def render_glyphs_to(self, writer: "NativeWriter", renderer: Renderer):
        """render_glyphs into a native sink (tar stream / directory)."""
        if _L().vg_manager_render_glyphs_to(self._h, renderer._h, writer._h) != 0:
            raise RuntimeError(_err())

    def write_index_json(self, writer: "NativeWriter"):
        if _L().vg_manager_write_index_json(self._h, writer._h) != 0:
            raise RuntimeError(_err())

    def write_families_json(self, writer: "NativeWriter"):
        if _L().vg_manager_write_families_json(self._h, writer._h) != 0:
            raise RuntimeError(_err())

    def shard_glyphs(self, font_id: str, world: int):
        """-> (owner u8[65536] with 0xFF = unmapped, estimated cost f64[65536]); SURVEY.md §8e."""
        owner = np.empty(65536, dtype=np.uint8)
        cost = np.empty(65536, dtype=np.float64)
        if _L().vg_manager_shard_glyphs(self._h, font_id.encode(), world, owner.ctypes.data, cost.ctypes.data) != 0:
            raise RuntimeError(_err())
        return owner, cost

    def plan_lanes(self, font_id: str, world: int):
        """-> (lane per code point u8[65536] with 0xFF = unmapped, number of this font's blocks split between lanes, the plan's own
        max / mean of the lanes' weights): what a run on `world` device lanes would do (no device needed)"""
        owner = np.empty(65536, dtype=np.uint8)
        n_split, ratio = C.c_uint32(0), C.c_double(0.0)
        if _L().vg_manager_plan_lanes(self._h, font_id.encode(), world, owner.ctypes.data, C.byref(n_split), C.byref(ratio)) != 0:
            raise RuntimeError(_err())
        return owner, int(n_split.value), float(ratio.value)

    def set_glyph_shard(self, rank: int, world: int):
        """Later render / build_batch calls see only rank's glyphs (world <= 1: off)."""
        if _L().vg_manager_set_glyph_shard(self._h, rank, world) != 0:
            raise RuntimeError(_err())

    def reduced_counters(self):
        """(blocks, glyphs, pixels) of the last render with a multi-device renderer, as reduced over its lanes"""
        out = (C.c_uint64 * 3)()
        _L().vg_manager_reduced_counters(self._h, out)
        return tuple(int(v) for v in out)

    def block_counts(self, font_id: str) -> np.ndarray:
        out = np.zeros(256, dtype=np.uint32)
        if _L().vg_manager_block_counts(self._h, font_id.encode(), out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
            raise KeyError(_err())
        return out

    def set_supplementary_planes(self, on: bool):
        """code points above U+FFFF (default off): one more block per populated range of 256 of them behind the 256 of the BMP"""
        if _L().vg_manager_set_supplementary_planes(self._h, int(bool(on))) != 0:
            raise RuntimeError(_err())

    def supplementary_blocks(self, font_id: str) -> dict:
        """{start: mapped code points} of the font id's supplementary blocks, ascending (empty with the switch off)"""
        n = _L().vg_manager_supplementary_blocks(self._h, font_id.encode(), None, None, 0)
        if n < 0:
            raise KeyError(_err())
        starts, counts = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        if _L().vg_manager_supplementary_blocks(self._h, font_id.encode(), starts.ctypes.data, counts.ctypes.data, n) != n:
            raise RuntimeError(_err())
        return {int(s): int(c) for s, c in zip(starts[:n], counts[:n])}

    def render_glyphs(self, writer, renderer: Renderer, font_id: str = None, block_starts=None):
        """FontManager::render_glyphs(&mut writer, &renderer).  `writer` needs
        write_directory(path) and write_file(path, bytes), or is None.  With font_id + block_starts only
        that shard of the (font, block) task list is rendered."""
        errors = []

        def cb(_user, path, data, n, is_dir):
            try:
                if is_dir:
                    writer.write_directory(path.decode())
                else:
                    writer.write_file(path.decode(), C.string_at(data, n) if n else b"")
                return 0
            except Exception as e:  # propagate through the C boundary as an abort
                errors.append(e)
                return 1

        # writer=None: NULL sink (the bytes are produced and counted, see timings()["pbf_bytes"], but not
        # handed to Python) -- what a native caller's in-memory writer costs
        ccb = WRITE_CB(cb) if writer is not None else C.cast(None, WRITE_CB)
        if block_starts is None:
            rc = _L().vg_manager_render_glyphs(self._h, renderer._h, ccb, None)
        else:
            arr = (C.c_uint32 * max(len(block_starts), 1))(*[int(b) for b in block_starts])
            rc = _L().vg_manager_render_blocks(self._h, renderer._h, font_id.encode(), arr, len(block_starts), ccb, None)
        if errors:
            raise errors[0]
        if rc != 0:
            raise RuntimeError(_err())

    def timings(self) -> dict:
        t = Timings()
        _L().vg_manager_timings(self._h, C.byref(t))
        return t.as_dict()

    def render_block(self, renderer: Renderer, font_id: str, start: int) -> bytes:
        """GlyphBlock::render(font_name, renderer) for block `start`."""
        need = _L().vg_manager_render_block(self._h, renderer._h, font_id.encode(), start, None, 0)
        if need < 0:
            raise RuntimeError(_err())
        out = np.empty(need, dtype=np.uint8)
        got = _L().vg_manager_render_block(self._h, renderer._h, font_id.encode(), start, out.ctypes.data, need)
        if got != need:
            raise RuntimeError(_err())
        return out.tobytes()

    def record_outlines(self, font_id: str) -> dict:
        """host half of the device front-end: {cmd_off, cmds, scale, shift_x, ids, advances} (numpy copies)"""
        h = _L().vg_manager_record_outlines(self._h, font_id.encode())
        if not h:
            raise RuntimeError(_err())
        try:
            co = _COutlines()
            ids, adv = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
            _L().vg_outline_batch_view(h, C.byref(co), C.byref(ids), C.byref(adv))
            n = co.n_glyphs

            def arr(ptr, count, dt):
                if count == 0 or not ptr:
                    return np.zeros(0, dtype=dt)
                buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
                return np.frombuffer(buf, dtype=dt, count=count).copy()

            cmd_off = arr(co.cmd_off, n + 1, np.uint32)
            return {"cmd_off": cmd_off, "cmds": arr(co.cmds, int(cmd_off[-1]) if n else 0, OUTLINE_CMD_DTYPE),
                    "scale": arr(co.scale, n, np.float64), "shift_x": arr(co.shift_x, n, np.float64),
                    "ids": arr(C.cast(ids, C.c_void_p).value, n, np.uint32),
                    "advances": arr(C.cast(adv, C.c_void_p).value, n, np.uint32)}
        finally:
            _L().vg_outline_batch_free(h)

    def record_glyf_parts(self, font_id: str) -> dict:
        """the same for the device's glyf decoder: {cmd_off (command slots), parts, bytes, scale, shift_x, ids, advances}"""
        from .device import GLYF_PART_DTYPE, _COutlinesGlyf
        L = _L()
        L.vg_manager_record_glyf_parts.restype = C.c_void_p
        L.vg_manager_record_glyf_parts.argtypes = [C.c_void_p, C.c_char_p]
        L.vg_glyf_batch_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vg_glyf_batch_free.argtypes = [C.c_void_p]
        L.vg_glyf_batch_free.restype = None
        h = L.vg_manager_record_glyf_parts(self._h, font_id.encode())
        if not h:
            raise RuntimeError(_err())
        try:
            co = _COutlinesGlyf()
            ids, adv = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
            L.vg_glyf_batch_view(h, C.byref(co), C.byref(ids), C.byref(adv))
            n = co.n_glyphs

            def arr(ptr, count, dt):
                if count == 0 or not ptr:
                    return np.zeros(0, dtype=dt)
                buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
                return np.frombuffer(buf, dtype=dt, count=count).copy()

            return {"cmd_off": arr(co.cmd_off, n + 1, np.uint32), "parts": arr(co.parts, co.n_parts, GLYF_PART_DTYPE),
                    "bytes": arr(co.bytes, co.n_bytes, np.uint8),
                    "scale": arr(co.scale, n, np.float64), "shift_x": arr(co.shift_x, n, np.float64),
                    "ids": arr(C.cast(ids, C.c_void_p).value, n, np.uint32),
                    "advances": arr(C.cast(adv, C.c_void_p).value, n, np.uint32)}
        finally:
            L.vg_glyf_batch_free(h)

    def resident_font_desc(self, font_id: str, file_index: int = 0) -> dict:
        """description of one file of a font id for vgsdf_font_create: {leaf_off, leaves, bytes} (numpy copies); every glyph
        id's leaves (cmd_at from the glyph's first slot), every simple glyph's arrays stored once"""
        from .device import GLYF_PART_DTYPE, _CFontDesc
        L = _L()
        L.vg_manager_resident_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d = _CFontDesc()
        if L.vg_manager_resident_font_desc(self._h, font_id.encode(), file_index, C.byref(d)) != 0:
            raise RuntimeError(_err())

        def arr(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count).copy()

        return {"leaf_off": arr(d.leaf_off, d.n_glyph_ids + 1, np.uint32), "leaves": arr(d.leaves, d.n_leaves, GLYF_PART_DTYPE),
                "bytes": arr(d.bytes, d.n_bytes, np.uint8)}

    def command_font_desc(self, font_id: str, file_index: int = 0) -> dict:
        """description of one file of a font id for vgsdf_font_create_commands: {cmd_off, dat_off, kinds, coords} (numpy
        copies); for every glyph id the callbacks the reader delivers, in the arrays of the packed form"""
        from .device import _CFontCmdsDesc
        L = _L()
        L.vg_manager_command_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d = _CFontCmdsDesc()
        if L.vg_manager_command_font_desc(self._h, font_id.encode(), file_index, C.byref(d)) != 0:
            raise RuntimeError(_err())

        def arr(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count).copy()

        return {"cmd_off": arr(d.cmd_off, d.n_glyph_ids + 1, np.uint32), "dat_off": arr(d.dat_off, d.n_glyph_ids + 1, np.uint32),
                "kinds": arr(d.kinds, d.n_cmds, np.uint8), "coords": arr(d.coords, d.n_floats, np.float32)}

    def charstring_font_desc(self, font_id: str, file_index: int = 0) -> dict:
        """description of one file of a font id for vgsdf_font_create_charstrings (vg_manager_charstring_font_desc; no device):
        {bytes, cs_off, gsubr_off, lsubr_first, lsubr_off, fd_of (None when there is one Font DICT)} as numpy copies.
        RuntimeError: a glyf face, a CFF2 face, a `CFF ` table the description cannot state"""
        from .device import _CFontCharstringsDesc
        L = _L()
        L.vg_manager_charstring_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d = _CFontCharstringsDesc()
        if L.vg_manager_charstring_font_desc(self._h, font_id.encode(), file_index, C.byref(d)) != 0:
            raise RuntimeError(_err())

        def arr(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count).copy()

        lsubr_first = arr(d.lsubr_first, d.n_fds + 1, np.uint32)
        return {"bytes": arr(d.bytes, d.n_bytes, np.uint8), "cs_off": arr(d.cs_off, d.n_glyph_ids + 1, np.uint32),
                "gsubr_off": arr(d.gsubr_off, d.n_gsubrs + 1, np.uint32), "lsubr_first": lsubr_first,
                "lsubr_off": arr(d.lsubr_off, int(lsubr_first[-1]) + 1, np.uint32),
                "fd_of": arr(d.fd_of, d.n_glyph_ids, np.uint8) if d.fd_of else None}

    def charstring2_font_desc(self, font_id: str, file_index: int = 0) -> dict:
        """description of one file of a font id for vgsdf_font_create_charstrings2 (vg_manager_charstring2_font_desc; no device):
        the keys of charstring_font_desc (fd_of None) plus the blend sets {set_ok, set_off, factors} as numpy copies.
        RuntimeError: anything that is not CFF2, a table the description cannot state"""
        from .device import _CFontCharstrings2Desc
        L = _L()
        L.vg_manager_charstring2_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d2 = _CFontCharstrings2Desc()
        if L.vg_manager_charstring2_font_desc(self._h, font_id.encode(), file_index, C.byref(d2)) != 0:
            raise RuntimeError(_err())
        d = d2.charstrings

        def arr(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count).copy()

        lsubr_first = arr(d.lsubr_first, d.n_fds + 1, np.uint32)
        return {"bytes": arr(d.bytes, d.n_bytes, np.uint8), "cs_off": arr(d.cs_off, d.n_glyph_ids + 1, np.uint32),
                "gsubr_off": arr(d.gsubr_off, d.n_gsubrs + 1, np.uint32), "lsubr_first": lsubr_first,
                "lsubr_off": arr(d.lsubr_off, int(lsubr_first[-1]) + 1, np.uint32), "fd_of": None,
                "set_ok": arr(d2.set_ok, d2.n_sets, np.uint8), "set_off": arr(d2.set_off, d2.n_sets + 1, np.uint32),
                "factors": arr(d2.factors, d2.n_factors, np.float32)}

    def charstring2_fonts_desc(self, font_id: str) -> dict:
        """the batched description of the instance group font_id's one file belongs to, for vgsdf_fonts_create_charstrings2
        (vg_manager_charstring2_fonts_desc; no device): the keys of charstring2_font_desc with "factors" the FIRST position's, plus
        "positions": float32 [n_positions, n_factors], the factors of every instance in the group's order — what
        Context.fonts_create_charstrings2 takes as (desc, positions).  RuntimeError: anything charstring2_font_desc refuses, a
        font id that is not in a group"""
        from .device import _CFontsCharstrings2Desc
        L = _L()
        ds = _CFontsCharstrings2Desc()
        if L.vg_manager_charstring2_fonts_desc(self._h, font_id.encode(), C.byref(ds)) != 0:
            raise RuntimeError(_err())
        d2, d = ds.face, ds.face.charstrings

        def arr(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count).copy()

        lsubr_first = arr(d.lsubr_first, d.n_fds + 1, np.uint32)
        positions = arr(d2.factors, d2.n_factors * ds.n_positions, np.float32).reshape(ds.n_positions, d2.n_factors)
        return {"bytes": arr(d.bytes, d.n_bytes, np.uint8), "cs_off": arr(d.cs_off, d.n_glyph_ids + 1, np.uint32),
                "gsubr_off": arr(d.gsubr_off, d.n_gsubrs + 1, np.uint32), "lsubr_first": lsubr_first,
                "lsubr_off": arr(d.lsubr_off, int(lsubr_first[-1]) + 1, np.uint32), "fd_of": None,
                "set_ok": arr(d2.set_ok, d2.n_sets, np.uint8), "set_off": arr(d2.set_off, d2.n_sets + 1, np.uint32),
                "factors": positions[0].copy() if ds.n_positions else np.zeros(0, dtype=np.float32), "positions": positions}

    def family_desc(self, font_id: str) -> dict:
        """the host half of a resident family (vg_manager_family_desc): {code_point, font_of, glyph_id, advance, scale, shift_x,
        n_files}, copies of the manager's table"""
        L = _L()
        v = _CFamilyView()
        if L.vg_manager_family_desc(self._h, font_id.encode(), C.byref(v)) != 0:
            raise RuntimeError(_err())
        n = v.n_entries

        def arr(ptr, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=n).copy()

        return {"code_point": arr(v.code_point, np.uint16), "font_of": arr(v.font_of, np.uint16), "glyph_id": arr(v.glyph_id, np.uint16),
                "advance": arr(v.advance, np.uint32), "scale": arr(v.scale, np.float64), "shift_x": arr(v.shift_x, np.float64),
                "n_files": int(v.n_files)}

    def family_tables_desc(self, font_id: str, file_index: int):
        """the description of one file's cmap and hmtx for SdfContext.family_create_tables (vg_manager_family_tables_desc), no
        device needed and no code point looked up: {cmap, hmtx (bytes), units_per_em, num_glyphs, num_hmetrics, subtable_off,
        subtable_format}, copies.  None: the description refuses (a cmap subtable that is not regular)"""
        L = _L()
        d = _CFaceTables()
        if L.vg_manager_family_tables_desc(self._h, font_id.encode(), int(file_index), C.byref(d)) != 0:
            if _err().startswith("refused"):
                return None
            raise RuntimeError(_err())
        n = d.n_subtables

        def arr(ptr, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            return np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt, count=n).copy()

        return {"cmap": C.string_at(d.cmap, d.cmap_len) if d.cmap_len else b"", "hmtx": C.string_at(d.hmtx, d.hmtx_len) if d.hmtx_len else b"",
                "units_per_em": int(d.units_per_em), "num_glyphs": int(d.num_glyphs), "num_hmetrics": int(d.num_hmetrics),
                "subtable_off": arr(d.subtable_off, np.uint32), "subtable_format": arr(d.subtable_format, np.uint16)}

    def font_position(self, font_id: str, file_index: int = 0):
        """the normalised coordinates (F2Dot14) a file was placed at (vg_manager_font_position); None: not at a position"""
        L = _L()
        n = L.vg_manager_font_position(self._h, font_id.encode(), int(file_index), None, 0)
        if n < 0:
            raise RuntimeError(_err())
        if n == 0:
            return None
        c = (C.c_int16 * n)()
        L.vg_manager_font_position(self._h, font_id.encode(), int(file_index), c, n)
        return [int(v) for v in c]

    def font_hor_advances(self, font_id: str, file_index: int = 0, extra: int = 0):
        """the reader's advance of every glyph id of a file, and of `extra` ids past numGlyphs, in font units
        (vg_manager_font_hor_advances; 0 for none)"""
        L = _L()
        n = L.vg_manager_font_hor_advances(self._h, font_id.encode(), int(file_index), None, 0)
        if n < 0:
            raise RuntimeError(_err())
        a = np.zeros(n + extra, np.uint16)
        L.vg_manager_font_hor_advances(self._h, font_id.encode(), int(file_index), a.ctypes.data, len(a))
        return a

    def font_gvar_advance_deltas(self, font_id: str, file_index: int = 0, extra: int = 0):
        """rule G7 for every glyph id of a glyf face placed by gvar, and `extra` ids past numGlyphs, whether or not its advances
        follow it (vg_manager_font_gvar_advance_deltas) -> (d: float32, state: uint8 — 0 none, 1 delta, 2 malformed)"""
        L = _L()
        n = L.vg_manager_font_gvar_advance_deltas(self._h, font_id.encode(), int(file_index), None, None, 0)
        if n < 0:
            raise RuntimeError(_err())
        d, st = np.zeros(n + extra, np.float32), np.zeros(n + extra, np.uint8)
        L.vg_manager_font_gvar_advance_deltas(self._h, font_id.encode(), int(file_index), d.ctypes.data, st.ctypes.data, len(d))
        return d, st

    def family_variation_desc(self, font_id: str, file_index: int):
        """what SdfContext.family_create_tables_var takes beside family_tables_desc for a file at a position
        (vg_manager_family_variation_desc): {hvar (bytes), store_off, map_off, region_scalars (float32)}, copies; {} for a file
        that is not at a position or has no HVAR (a static face).  None: the description refuses"""
        d = _CFaceVariation()
        if _L().vg_manager_family_variation_desc(self._h, font_id.encode(), int(file_index), C.byref(d)) != 0:
            if _err().startswith("refused"):
                return None
            raise RuntimeError(_err())
        if not d.hvar:
            return {}
        sc = np.frombuffer((C.c_char * (4 * d.n_regions)).from_address(d.region_scalars), dtype=np.float32, count=d.n_regions).copy() \
            if d.n_regions else np.zeros(0, np.float32)
        return {"hvar": C.string_at(d.hvar, d.hvar_len), "store_off": int(d.store_off), "map_off": int(d.map_off), "region_scalars": sc}

    def font_tables_desc(self, font_id: str, file_index: int = 0):
        """the description of one file's loca and glyf for SdfContext.font_create_tables (vg_manager_font_tables_desc), no device
        needed and no glyph looked at: {loca, glyf (bytes), num_glyphs, loca_entries, loca_long}, copies.  None: the description
        refuses (a face without glyf outlines)"""
        from .device import _CFontTablesDesc
        L = _L()
        L.vg_manager_font_tables_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d = _CFontTablesDesc()
        if L.vg_manager_font_tables_desc(self._h, font_id.encode(), int(file_index), C.byref(d)) != 0:
            if _err().startswith("refused"):
                return None
            raise RuntimeError(_err())
        return {"loca": C.string_at(d.loca, d.n_loca_bytes) if d.n_loca_bytes else b"", "glyf": C.string_at(d.glyf, d.n_glyf_bytes) if d.n_glyf_bytes else b"",
                "num_glyphs": int(d.num_glyphs), "loca_entries": int(d.loca_entries), "loca_long": int(d.loca_long)}

    def gvar_font_desc(self, font_id: str, file_index: int = 0):
        """the description of one placed `glyf` file for SdfContext.font_create_gvar (vg_manager_gvar_font_desc), no device needed
        and no glyph looked at: the keys of font_tables_desc plus gvar (bytes) and coords (int16 per axis), copies.  None: the
        description refuses (not a glyf face placed by gvar)"""
        from .device import _CFontGvarDesc
        L = _L()
        L.vg_manager_gvar_font_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d = _CFontGvarDesc()
        if L.vg_manager_gvar_font_desc(self._h, font_id.encode(), int(file_index), C.byref(d)) != 0:
            if _err().startswith("refused"):
                return None
            raise RuntimeError(_err())
        t = d.tables
        return {"loca": C.string_at(t.loca, t.n_loca_bytes) if t.n_loca_bytes else b"", "glyf": C.string_at(t.glyf, t.n_glyf_bytes) if t.n_glyf_bytes else b"",
                "num_glyphs": int(t.num_glyphs), "loca_entries": int(t.loca_entries), "loca_long": int(t.loca_long),
                "gvar": C.string_at(d.gvar, d.gvar_len), "coords": np.frombuffer(C.string_at(d.coords, 2 * d.n_axes), dtype=np.int16).copy()}

    def family_gvar_desc(self, font_id: str, file_index: int = 0):
        """what SdfContext.family_create_tables_gvar takes beside family_tables_desc and family_variation_desc
        (vg_manager_family_gvar_desc): the dict of gvar_font_desc for a face whose advances follow gvar's phantom points, None for
        every other face"""
        from .device import _CFontGvarDesc
        L = _L()
        L.vg_manager_family_gvar_desc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        d = _CFontGvarDesc()
        if L.vg_manager_family_gvar_desc(self._h, font_id.encode(), int(file_index), C.byref(d)) != 0:
            raise RuntimeError(_err())
        return self.gvar_font_desc(font_id, file_index) if d.gvar else None

    def record_resident_commands(self, font_id: str) -> dict:
        """record_resident against command fonts: for any face the reader can read (CFF, CFF2, glyf)"""
        return self.record_resident(font_id, _commands=True)

    def record_resident(self, font_id: str, _commands: bool = False) -> dict:
        """what a resident submission of the font names: {font_of, glyph_id, scale, shift_x, ids, advances, n_files}"""
        L = _L()
        L.vg_manager_record_resident.restype = C.c_void_p
        L.vg_manager_record_resident.argtypes = [C.c_void_p, C.c_char_p]
        L.vg_manager_record_resident_commands.restype = C.c_void_p
        L.vg_manager_record_resident_commands.argtypes = [C.c_void_p, C.c_char_p]
        L.vg_resident_batch_view.argtypes = [C.c_void_p, C.c_void_p]
        L.vg_resident_batch_free.argtypes = [C.c_void_p]
        L.vg_resident_batch_free.restype = None
        h = (L.vg_manager_record_resident_commands if _commands else L.vg_manager_record_resident)(self._h, font_id.encode())
        if not h:
            raise RuntimeError(_err())
        try:
            v = _CResidentView()
            L.vg_resident_batch_view(h, C.byref(v))
            n = v.n_glyphs

            def arr(ptr, dt):
                if n == 0 or not ptr:
                    return np.zeros(0, dtype=dt)
                buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
                return np.frombuffer(buf, dtype=dt, count=n).copy()

            return {"font_of": arr(v.font_of, np.uint16), "glyph_id": arr(v.glyph_id, np.uint16), "scale": arr(v.scale, np.float64),
                    "shift_x": arr(v.shift_x, np.float64), "ids": arr(v.ids, np.uint32), "advances": arr(v.advances, np.uint32),
                    "n_files": int(v.n_files)}
        finally:
            L.vg_resident_batch_free(h)

    def build_batch(self, font_id: str) -> GlyphBatchHost:
        h = _L().vg_manager_build_batch(self._h, font_id.encode())
        if not h:
            raise RuntimeError(_err())
        return GlyphBatchHost(h)

    def close(self):
        if self._h:
            _L().vg_manager_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeWriter:
    """src/writer: Writer::new_tar / Writer::new_file, implemented natively (csrc/host/writers.cpp)."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError(_err())
        self._h = handle

    @classmethod
    def new_tar(cls, path, mtime: int = -1):
        return cls(_L().vg_writer_new_tar_path(str(path).encode(), mtime))

    @classmethod
    def new_tar_fd(cls, fd: int, mtime: int = -1):
        return cls(_L().vg_writer_new_tar_fd(fd, mtime))

    @classmethod
    def new_file(cls, folder):
        return cls(_L().vg_writer_new_dir(str(folder).encode()))

    def write_file(self, path: str, data: bytes):
        if _L().vg_writer_write_file(self._h, path.encode(), data, len(data)) != 0:
            raise RuntimeError(_err())

    def write_directory(self, path: str):
        if _L().vg_writer_write_directory(self._h, path.encode()) != 0:
            raise RuntimeError(_err())

    def finish(self):
        if _L().vg_writer_finish(self._h) != 0:
            raise RuntimeError(_err())

    def close(self):
        if self._h:
            _L().vg_writer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pbf_merge(parts, consecutive: bool = False) -> bytes:
    """Partial PBFs of one block (disjoint glyph subsets) -> the block's PBF.  consecutive=True: vg_pbf_concat (parts that
    hold consecutive runs of the block's code points, in order)."""
    parts = [bytes(p) for p in parts]
    fn = _L().vg_pbf_concat if consecutive else _L().vg_pbf_merge
    arr = (C.c_char_p * len(parts))(*parts)
    lens = (C.c_size_t * len(parts))(*[len(p) for p in parts])
    need = fn(arr, lens, len(parts), None, 0)
    if need < 0:
        raise RuntimeError(_err())
    out = np.empty(need, dtype=np.uint8)
    fn(arr, lens, len(parts), out.ctypes.data, need)
    return out.tobytes()


def parse_font_name(family: str, ps_name: str):
    """(family, style, weight, width) — src/font/parse_font_name.rs:214-291"""
    fam = C.create_string_buffer(1024)
    style = C.create_string_buffer(16)
    width = C.create_string_buffer(16)
    weight = C.c_uint16(0)
    _L().vg_parse_font_name(family.encode(), ps_name.encode(), fam, len(fam), style, C.byref(weight), width)
    return fam.value.decode(), style.value.decode(), int(weight.value), width.value.decode()


def encode_codeblocks(codepoints) -> str:
    """src/font/index_files.rs:65-103"""
    cps = np.ascontiguousarray(codepoints, dtype=np.uint32)
    need = _L().vg_encode_codeblocks(cps.ctypes.data, cps.size, None, 0)
    buf = C.create_string_buffer(need)
    _L().vg_encode_codeblocks(cps.ctypes.data, cps.size, buf, need)
    return buf.value.decode()


class DummyWriter:
    """src/writer/dummy.rs: records 'name (len)' strings; keeps the bytes too."""

    def __init__(self):
        self.inner, self.files = [], {}

    def write_directory(self, path):
        self.inner.append(path)

    def write_file(self, path, data):
        self.inner.append(f"{path} ({len(data)})")
        self.files[path] = data


def pbf_encode(name: str, range_: str, glyphs) -> bytes:
    """glyphs: [PbfGlyph] (bitmap attribute used when has_bitmap)."""
    n = len(glyphs)
    arr = (PbfGlyph * max(n, 1))()
    ptrs = (C.c_void_p * max(n, 1))()
    keep = []
    for i, g in enumerate(glyphs):
        arr[i] = g
        if g.has_bitmap and g.bitmap is not None:
            b = np.ascontiguousarray(g.bitmap, dtype=np.uint8)
            keep.append(b)
            arr[i].bitmap_len = b.size
            ptrs[i] = b.ctypes.data
    need = _L().vg_pbf_encode(name.encode(), range_.encode(), arr, ptrs, n, None, 0)
    out = np.empty(need, dtype=np.uint8)
    _L().vg_pbf_encode(name.encode(), range_.encode(), arr, ptrs, n, out.ctypes.data, need)
    return out.tobytes()
