"""ctypes binding of include/vgsdf.h (the device boundary)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .build import lib_path


class VgsdfError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vgsdf error {code}: {msg}")
        self.code = code


class _CBatch(C.Structure):
    _fields_ = [("n_glyphs", C.c_uint32), ("seg_off", C.c_void_p), ("seg_sx", C.c_void_p),
                ("seg_sy", C.c_void_p), ("seg_ex", C.c_void_p), ("seg_ey", C.c_void_p),
                ("x0", C.c_void_p), ("y0", C.c_void_p), ("w", C.c_void_p), ("h", C.c_void_p),
                ("out_off", C.c_void_p)]


class _CStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_glyphs", "n_segments", "n_pixels", "n_pairs", "n_tiles", "alg_bytes")]


OUTLINE_CMD_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("x", "<f4"), ("y", "<f4"),
                              ("kind", "<u4")])
RECT_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<u4"), ("h", "<u4"), ("n_segments", "<u4"),
                       ("has_raster", "<u4")])


class _COutlines(C.Structure):
    _fields_ = [("n_glyphs", C.c_uint32), ("cmd_off", C.c_void_p), ("cmds", C.c_void_p), ("scale", C.c_void_p),
                ("shift_x", C.c_void_p)]


class _COutlinesPacked(C.Structure):
    _fields_ = [("n_glyphs", C.c_uint32), ("cmd_off", C.c_void_p), ("dat_off", C.c_void_p), ("kinds", C.c_void_p),
                ("coords", C.c_void_p), ("scale", C.c_void_p), ("shift_x", C.c_void_p),
                ("pbf_pre", C.c_void_p), ("pbf_fix", C.c_void_p)]  # in-place PBF assembly: NULL = bitmaps packed back to back


class _COutlinesGlyf(C.Structure):
    _fields_ = [("n_glyphs", C.c_uint32), ("n_parts", C.c_uint32), ("n_bytes", C.c_uint32), ("cmd_off", C.c_void_p),
                ("parts", C.c_void_p), ("bytes", C.c_void_p), ("scale", C.c_void_p), ("shift_x", C.c_void_p),
                ("pbf_pre", C.c_void_p), ("pbf_fix", C.c_void_p)]


# vgsdf_glyf_part: one simple glyph of a (possibly composite) glyph for the device's glyf decoder
GLYF_PART_DTYPE = np.dtype([("byte_off", "<u4"), ("byte_len", "<u4"), ("cmd_at", "<u4"), ("cmd_cap", "<u4"), ("n_contours", "<u4"),
                            ("plain", "<u4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("d", "<f4"), ("e", "<f4"), ("f", "<f4")])
VGSDF_E_ARG = -1
VGSDF_E_GLYF = -4


class _CFontDesc(C.Structure):  # vgsdf_font_desc
    _fields_ = [("n_glyph_ids", C.c_uint32), ("n_leaves", C.c_uint32), ("n_bytes", C.c_uint32), ("leaf_off", C.c_void_p),
                ("leaves", C.c_void_p), ("bytes", C.c_void_p)]


class _CFontCmdsDesc(C.Structure):  # vgsdf_font_cmds_desc
    _fields_ = [("n_glyph_ids", C.c_uint32), ("n_cmds", C.c_uint32), ("n_floats", C.c_uint32), ("cmd_off", C.c_void_p),
                ("dat_off", C.c_void_p), ("kinds", C.c_void_p), ("coords", C.c_void_p)]


class _CFontCharstringsDesc(C.Structure):  # vgsdf_font_charstrings_desc
    _fields_ = [("n_glyph_ids", C.c_uint32), ("n_bytes", C.c_uint32), ("bytes", C.c_void_p), ("cs_off", C.c_void_p),
                ("n_gsubrs", C.c_uint32), ("gsubr_off", C.c_void_p), ("n_fds", C.c_uint32), ("lsubr_first", C.c_void_p),
                ("lsubr_off", C.c_void_p), ("fd_of", C.c_void_p)]


class _CFontCharstrings2Desc(C.Structure):  # vgsdf_font_charstrings2_desc
    _fields_ = [("charstrings", _CFontCharstringsDesc), ("n_sets", C.c_uint32), ("n_factors", C.c_uint32), ("set_ok", C.c_void_p),
                ("set_off", C.c_void_p), ("factors", C.c_void_p)]


class _CFontsCharstrings2Desc(C.Structure):  # vgsdf_fonts_charstrings2_desc
    _fields_ = [("face", _CFontCharstrings2Desc), ("n_positions", C.c_uint32)]


class _COutlinesResident(C.Structure):  # vgsdf_outlines_resident
    _fields_ = [("n_glyphs", C.c_uint32), ("n_fonts", C.c_uint32), ("fonts", C.c_void_p), ("font_of", C.c_void_p),
                ("glyph_id", C.c_void_p), ("scale", C.c_void_p), ("shift_x", C.c_void_p), ("pbf_pre", C.c_void_p),
                ("pbf_fix", C.c_void_p)]

class _CFamilyDesc(C.Structure):  # vgsdf_family_desc
    _fields_ = [("n_fonts", C.c_uint32), ("fonts", C.c_void_p), ("n_entries", C.c_uint32), ("code_point", C.c_void_p),
                ("font_of", C.c_void_p), ("glyph_id", C.c_void_p), ("advance", C.c_void_p), ("scale", C.c_void_p), ("shift_x", C.c_void_p)]


class _CFaceTables(C.Structure):  # vgsdf_face_tables
    _fields_ = [("cmap", C.c_void_p), ("cmap_len", C.c_uint32), ("hmtx", C.c_void_p), ("hmtx_len", C.c_uint32),
                ("units_per_em", C.c_uint16), ("num_glyphs", C.c_uint16), ("num_hmetrics", C.c_uint16), ("n_subtables", C.c_uint16),
                ("subtable_off", C.c_void_p), ("subtable_format", C.c_void_p)]


class _CFaceVariation(C.Structure):  # vgsdf_face_variation
    _fields_ = [("hvar", C.c_void_p), ("hvar_len", C.c_uint32), ("store_off", C.c_uint32), ("map_off", C.c_uint32),
                ("region_scalars", C.c_void_p), ("n_regions", C.c_uint32)]


class _CFamilyTablesDesc(C.Structure):  # vgsdf_family_tables_desc
    _fields_ = [("n_fonts", C.c_uint32), ("fonts", C.c_void_p), ("tables", C.c_void_p)]


class _CFamiliesTablesDesc(C.Structure):  # vgsdf_families_tables_desc
    _fields_ = [("n_positions", C.c_uint32), ("fonts", C.c_void_p), ("tables", _CFaceTables), ("var", C.c_void_p), ("gvar", C.c_void_p)]


class _CFontTablesDesc(C.Structure):  # vgsdf_font_tables_desc
    _fields_ = [("num_glyphs", C.c_uint32), ("loca_entries", C.c_uint32), ("loca_long", C.c_uint32), ("n_loca_bytes", C.c_uint32),
                ("n_glyf_bytes", C.c_uint32), ("loca", C.c_void_p), ("glyf", C.c_void_p)]


class _CFontGvarDesc(C.Structure):  # vgsdf_font_gvar_desc
    _fields_ = [("tables", _CFontTablesDesc), ("gvar", C.c_void_p), ("gvar_len", C.c_uint32), ("n_axes", C.c_uint32), ("coords", C.c_void_p)]


class _CFontsGvarDesc(C.Structure):  # vgsdf_fonts_gvar_desc
    _fields_ = _CFontGvarDesc._fields_ + [("n_positions", C.c_uint32)]


class _COutlinesRanges(C.Structure):  # vgsdf_outlines_ranges
    _fields_ = [("n_tasks", C.c_uint32), ("n_families", C.c_uint32), ("families", C.c_void_p), ("family_of", C.c_void_p),
                ("first", C.c_void_p), ("last", C.c_void_p), ("pbf_pre", C.c_void_p)]


VGSDF_SYMBOLS = [
    "vgsdf_device_count", "vgsdf_create", "vgsdf_destroy", "vgsdf_last_error", "vgsdf_render_batch",
    "vgsdf_batch_upload", "vgsdf_batch_launch", "vgsdf_batch_download", "vgsdf_batch_free", "vgsdf_sync",
    "vgsdf_batch_stats", "vgsdf_batch_time", "vgsdf_set_variant", "vgsdf_batch_device_output",
    "vgsdf_host_alloc", "vgsdf_host_free", "vgsdf_outlines_prepare", "vgsdf_outlines_render", "vgsdf_outlines_render_into", "vgsdf_outlines_submit", "vgsdf_outlines_submit_packed", "vgsdf_outlines_submit_glyf", "vgsdf_outlines_wait", "vgsdf_outlines_segments",
    "vgsdf_add_counters", "vgsdf_reset_counters", "vgsdf_reduce_counters", "vgsdf_reduce_counters_rccl", "vgsdf_reduce_path", "vgsdf_outlines_pbf_positions", "vgsdf_outlines_peek",
    "vgsdf_font_create", "vgsdf_font_free", "vgsdf_font_device_bytes", "vgsdf_outlines_submit_resident", "vgsdf_outlines_resident_upload_bytes",
    "vgsdf_font_create_commands", "vgsdf_font_create_charstrings", "vgsdf_font_create_charstrings_within", "vgsdf_font_create_charstrings2", "vgsdf_font_create_charstrings2_within", "vgsdf_font_charstrings_kernel_ms", "vgsdf_font_commands_read",
    "vgsdf_fonts_create_charstrings2", "vgsdf_fonts_create_charstrings2_within", "vgsdf_fonts_charstrings2_kernel_ms",
    "vgsdf_family_create", "vgsdf_family_free", "vgsdf_family_device_bytes", "vgsdf_family_count", "vgsdf_outlines_submit_ranges",
    "vgsdf_outlines_task_extents", "vgsdf_family_create_tables", "vgsdf_family_read", "vgsdf_family_tables_kernel_ms",
    "vgsdf_font_create_tables", "vgsdf_font_create_tables_within", "vgsdf_font_read", "vgsdf_font_tables_kernel_ms",
    "vgsdf_fonts_create_tables", "vgsdf_fonts_create_tables_within", "vgsdf_fonts_tables_kernel_ms",
    "vgsdf_font_create_gvar", "vgsdf_font_create_gvar_within", "vgsdf_font_gvar_kernel_ms",
    "vgsdf_fonts_create_gvar", "vgsdf_fonts_create_gvar_within", "vgsdf_fonts_gvar_kernel_ms",
    "vgsdf_outlines_submit_resident_mixed", "vgsdf_family_create_mixed", "vgsdf_family_create_tables_mixed",
    "vgsdf_family_create_tables_var", "vgsdf_family_create_tables_var_mixed",
    "vgsdf_gvar_advance_deltas", "vgsdf_gvar_advance_kernel_ms", "vgsdf_family_create_tables_gvar", "vgsdf_family_create_tables_gvar_mixed",
    "vgsdf_families_create_tables", "vgsdf_families_create_tables_mixed", "vgsdf_gvar_advance_deltas_batch", "vgsdf_families_tables_kernel_ms",
    "vgsdf_batch_union", "vgsdf_batch_segments_read", "vgsdf_outlines_union", "vgsdf_union_kernel_ms",
    "vgsdf_family_create_at", "vgsdf_family_create_tables_at", "vgsdf_family_plane", "vgsdf_family_tables_census", "vgsdf_family_census_kernel_ms",
]

_lib = None


def load_library():
    """dlopen libvgsdf.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not p.exists():
            raise FileNotFoundError(f"{p} missing: run __graft_entry__.build() (hipcc) first; "
                                    "there is no CPU fallback")
        L = C.CDLL(str(p))
        vp = C.c_void_p
        L.vgsdf_device_count.restype = C.c_int
        L.vgsdf_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.vgsdf_destroy.argtypes = [vp]
        L.vgsdf_destroy.restype = None
        L.vgsdf_last_error.argtypes = [vp]
        L.vgsdf_last_error.restype = C.c_char_p
        L.vgsdf_render_batch.argtypes = [vp, C.POINTER(_CBatch), vp]
        L.vgsdf_batch_upload.argtypes = [vp, C.POINTER(_CBatch), C.POINTER(vp)]
        L.vgsdf_batch_launch.argtypes = [vp, vp]
        L.vgsdf_batch_download.argtypes = [vp, vp, vp]
        L.vgsdf_batch_free.argtypes = [vp, vp]
        L.vgsdf_sync.argtypes = [vp]
        L.vgsdf_batch_stats.argtypes = [vp, C.POINTER(_CStats)]
        L.vgsdf_batch_time.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_float)]
        L.vgsdf_set_variant.argtypes = [vp, C.c_int]
        L.vgsdf_batch_device_output.argtypes = [vp]
        L.vgsdf_batch_device_output.restype = vp
        L.vgsdf_host_alloc.argtypes = [C.c_size_t]
        L.vgsdf_host_alloc.restype = vp
        L.vgsdf_host_free.argtypes = [vp]
        L.vgsdf_host_free.restype = None
        L.vgsdf_outlines_prepare.argtypes = [vp, C.POINTER(_COutlines), vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.vgsdf_outlines_render.argtypes = [vp, vp]
        L.vgsdf_outlines_render_into.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
        L.vgsdf_outlines_submit.argtypes = [vp, vp, vp, C.c_size_t]
        L.vgsdf_outlines_wait.argtypes = [vp, vp, vp, vp, vp]
        L.vgsdf_outlines_submit_packed.argtypes = [vp, vp, vp, C.c_size_t]
        L.vgsdf_outlines_submit_glyf.argtypes = [vp, vp, vp, C.c_size_t]
        L.vgsdf_outlines_segments.argtypes = [vp, vp, vp, vp, vp, vp]
        L.vgsdf_batch_union.argtypes = [vp, vp, C.POINTER(vp), vp]
        L.vgsdf_batch_segments_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.vgsdf_outlines_union.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
        L.vgsdf_union_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_union_kernel_ms.restype = None
        L.vgsdf_outlines_pbf_positions.argtypes = [vp, vp]
        L.vgsdf_outlines_peek.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.vgsdf_font_create.argtypes = [vp, C.POINTER(_CFontDesc), C.POINTER(vp)]
        L.vgsdf_font_create_commands.argtypes = [vp, C.POINTER(_CFontCmdsDesc), C.POINTER(vp)]
        L.vgsdf_font_create_charstrings.argtypes = [vp, C.POINTER(_CFontCharstringsDesc), C.POINTER(vp)]
        L.vgsdf_font_create_charstrings_within.argtypes = [vp, C.POINTER(_CFontCharstringsDesc), C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.vgsdf_font_create_charstrings2.argtypes = [vp, C.POINTER(_CFontCharstrings2Desc), C.POINTER(vp)]
        L.vgsdf_font_create_charstrings2_within.argtypes = [vp, C.POINTER(_CFontCharstrings2Desc), C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.vgsdf_font_charstrings_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_font_charstrings_kernel_ms.restype = None
        L.vgsdf_fonts_create_charstrings2.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vgsdf_fonts_create_charstrings2_within.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vgsdf_fonts_charstrings2_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_fonts_charstrings2_kernel_ms.restype = None
        L.vgsdf_font_commands_read.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, vp, vp]
        L.vgsdf_font_create_tables.argtypes = [vp, C.POINTER(_CFontTablesDesc), C.POINTER(vp)]
        L.vgsdf_font_create_tables_within.argtypes = [vp, C.POINTER(_CFontTablesDesc), C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.vgsdf_font_read.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, vp, vp]
        L.vgsdf_font_tables_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_font_tables_kernel_ms.restype = None
        L.vgsdf_fonts_create_tables.argtypes = [vp, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.vgsdf_fonts_create_tables_within.argtypes = [vp, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vgsdf_fonts_tables_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_fonts_tables_kernel_ms.restype = None
        L.vgsdf_font_create_gvar.argtypes = [vp, C.POINTER(_CFontGvarDesc), C.POINTER(vp)]
        L.vgsdf_font_create_gvar_within.argtypes = [vp, C.POINTER(_CFontGvarDesc), C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.vgsdf_font_gvar_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_font_gvar_kernel_ms.restype = None
        L.vgsdf_fonts_create_gvar.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vgsdf_fonts_create_gvar_within.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vgsdf_fonts_gvar_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_fonts_gvar_kernel_ms.restype = None
        L.vgsdf_font_free.argtypes = [vp, vp]
        L.vgsdf_font_device_bytes.argtypes = [vp]
        L.vgsdf_font_device_bytes.restype = C.c_uint64
        L.vgsdf_outlines_submit_resident.argtypes = [vp, vp, vp, C.c_size_t]
        L.vgsdf_outlines_submit_resident_mixed.argtypes = [vp, vp, vp, C.c_size_t]
        L.vgsdf_outlines_resident_upload_bytes.argtypes = [vp]
        L.vgsdf_outlines_resident_upload_bytes.restype = C.c_uint64
        L.vgsdf_family_create.argtypes = [vp, C.POINTER(_CFamilyDesc), C.POINTER(vp)]
        L.vgsdf_family_create_mixed.argtypes = [vp, C.POINTER(_CFamilyDesc), C.POINTER(vp)]
        L.vgsdf_family_create_tables_mixed.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), C.POINTER(vp)]
        L.vgsdf_family_create_at.argtypes = [vp, C.POINTER(_CFamilyDesc), C.c_int, C.c_uint32, C.POINTER(vp)]
        L.vgsdf_family_create_tables_at.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), C.c_int, C.c_uint32, C.POINTER(vp)]
        L.vgsdf_family_plane.argtypes = [vp]
        L.vgsdf_family_tables_census.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), vp]
        L.vgsdf_family_census_kernel_ms.argtypes = [vp]
        L.vgsdf_family_census_kernel_ms.restype = C.c_float
        L.vgsdf_family_plane.restype = C.c_uint32
        L.vgsdf_family_free.argtypes = [vp, vp]
        L.vgsdf_family_device_bytes.argtypes = [vp]
        L.vgsdf_family_device_bytes.restype = C.c_uint64
        L.vgsdf_family_count.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.vgsdf_family_count.restype = C.c_uint32
        L.vgsdf_family_create_tables.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), C.POINTER(vp)]
        L.vgsdf_family_create_tables_var.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), vp, C.POINTER(vp)]
        L.vgsdf_family_create_tables_var_mixed.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), vp, C.POINTER(vp)]
        L.vgsdf_family_create_tables_gvar.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), vp, vp, C.POINTER(vp)]
        L.vgsdf_family_create_tables_gvar_mixed.argtypes = [vp, C.POINTER(_CFamilyTablesDesc), vp, vp, C.POINTER(vp)]
        L.vgsdf_gvar_advance_deltas.argtypes = [vp, C.POINTER(_CFontGvarDesc), vp, vp]
        L.vgsdf_gvar_advance_kernel_ms.argtypes = [vp]
        L.vgsdf_gvar_advance_kernel_ms.restype = C.c_float
        L.vgsdf_families_create_tables.argtypes = [vp, vp, vp, vp]
        L.vgsdf_families_create_tables_mixed.argtypes = [vp, vp, vp, vp]
        L.vgsdf_gvar_advance_deltas_batch.argtypes = [vp, vp, vp, vp]
        L.vgsdf_families_tables_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_families_tables_kernel_ms.restype = None
        L.vgsdf_family_read.argtypes = [vp, vp, C.POINTER(C.c_uint32)] + [vp] * 9
        L.vgsdf_family_tables_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.vgsdf_family_tables_kernel_ms.restype = None
        L.vgsdf_outlines_submit_ranges.argtypes = [vp, vp, vp, C.c_size_t]
        L.vgsdf_outlines_task_extents.argtypes = [vp, vp]
        L.vgsdf_add_counters.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64]
        L.vgsdf_add_counters.restype = None
        L.vgsdf_reset_counters.argtypes = [vp]
        L.vgsdf_reset_counters.restype = None
        L.vgsdf_reduce_counters.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_uint64)]
        L.vgsdf_reduce_counters_rccl.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_uint64)]
        L.vgsdf_reduce_path.argtypes = [vp]
        L.vgsdf_reduce_path.restype = C.c_char_p
        _lib = L
    return _lib


def device_count() -> int:
    return load_library().vgsdf_device_count()


def reduce_counters(contexts, strict=False):
    """vgsdf_reduce_counters: (blocks, glyphs, pixels) summed over the contexts' run counters — an RCCL all-reduce when
    two or more contexts sit on distinct devices, with the host's own sum as the flagged fallback (reduce_path tells);
    strict=True: vgsdf_reduce_counters_rccl — through RCCL or an error (a single context: a communicator of one rank)."""
    L = load_library()
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    out = (C.c_uint64 * 3)()
    rc = (L.vgsdf_reduce_counters_rccl if strict else L.vgsdf_reduce_counters)(arr, len(contexts), out)
    if rc != 0:
        raise VgsdfError(rc, (L.vgsdf_last_error(contexts[0]._h) or b"").decode())
    return tuple(int(v) for v in out)


def reduce_path(context) -> str:
    """vgsdf_reduce_path: "rccl", "host: one context", "host: contexts share a device" or "host: RCCL fallback: <reason>" """
    return (load_library().vgsdf_reduce_path(context._h) or b"").decode()


@dataclass
class Batch:
    """Host SoA batch (vgsdf_batch).  Arrays are kept alive by this object."""
    seg_off: np.ndarray  # u32 [n+1]
    seg_sx: np.ndarray   # f64 [S]
    seg_sy: np.ndarray
    seg_ex: np.ndarray
    seg_ey: np.ndarray
    x0: np.ndarray       # i32 [n]
    y0: np.ndarray
    w: np.ndarray        # u32 [n]
    h: np.ndarray
    out_off: np.ndarray  # u64 [n+1]

    @property
    def n_glyphs(self) -> int:
        return len(self.w)

    @property
    def out_bytes(self) -> int:
        return int(self.out_off[-1]) if len(self.out_off) else 0

    def c_struct(self) -> _CBatch:
        p = lambda a: a.ctypes.data  # noqa: E731
        return _CBatch(self.n_glyphs, p(self.seg_off), p(self.seg_sx), p(self.seg_sy), p(self.seg_ex),
                       p(self.seg_ey), p(self.x0), p(self.y0), p(self.w), p(self.h), p(self.out_off))

    def bitmap(self, out: np.ndarray, g: int) -> np.ndarray:
        a, b = int(self.out_off[g]), int(self.out_off[g + 1])
        return out[a:b].reshape(int(self.h[g]), int(self.w[g]))


def make_batch(glyphs) -> Batch:
    """glyphs: iterable of (segs[n,4] f64 (sx,sy,ex,ey), x0, y0, w, h)."""
    glyphs = list(glyphs)
    n = len(glyphs)
    seg_off = np.zeros(n + 1, dtype=np.uint32)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    x0 = np.zeros(n, dtype=np.int32)
    y0 = np.zeros(n, dtype=np.int32)
    w = np.zeros(n, dtype=np.uint32)
    h = np.zeros(n, dtype=np.uint32)
    parts = []
    for i, (segs, gx0, gy0, gw, gh) in enumerate(glyphs):
        segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4)
        parts.append(segs)
        seg_off[i + 1] = seg_off[i] + len(segs)
        out_off[i + 1] = out_off[i] + np.uint64(int(gw) * int(gh))
        x0[i], y0[i], w[i], h[i] = gx0, gy0, gw, gh
    allseg = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4))
    col = lambda k: np.ascontiguousarray(allseg[:, k])  # noqa: E731
    return Batch(seg_off, col(0), col(1), col(2), col(3), x0, y0, w, h, out_off)


class DeviceBatch:
    """A batch resident in HBM (vgsdf_dbatch)."""

    def __init__(self, ctx: "SdfContext", handle, out_bytes: int):
        self.ctx, self._h, self.out_bytes = ctx, handle, out_bytes

    def launch(self):
        self.ctx._check(load_library().vgsdf_batch_launch(self.ctx._h, self._h))

    def download(self) -> np.ndarray:
        out = np.empty(self.out_bytes, dtype=np.uint8)
        self.ctx._check(load_library().vgsdf_batch_download(self.ctx._h, self._h, out.ctypes.data))
        return out

    def time(self, iters: int) -> float:
        """total milliseconds for `iters` launches (HIP events on the context stream)."""
        ms = C.c_float(0)
        self.ctx._check(load_library().vgsdf_batch_time(self.ctx._h, self._h, iters, C.byref(ms)))
        return float(ms.value)

    def stats(self) -> dict:
        s = _CStats()
        load_library().vgsdf_batch_stats(self._h, C.byref(s))
        return {k: int(getattr(s, k)) for k, _ in _CStats._fields_}

    def device_output_ptr(self) -> int:
        return int(load_library().vgsdf_batch_device_output(self._h) or 0)

    def union(self):
        """vgsdf_batch_union: rule U over this batch -> (a NEW DeviceBatch of the same glyphs and rects whose segments are
        the boundary of the filled sets, state u8[n_glyphs]: 0 identity, 1 rebuilt, 2 over the limit, 3 non-finite)"""
        state = np.zeros(self.stats()["n_glyphs"], dtype=np.uint8)
        h = C.c_void_p()
        self.ctx._check(load_library().vgsdf_batch_union(self.ctx._h, self._h, C.byref(h), state.ctypes.data))
        return DeviceBatch(self.ctx, h, self.out_bytes), state

    def segments(self):
        """vgsdf_batch_segments_read -> (seg_off[n+1], segs[S,4])"""
        L = load_library()
        seg_off = np.zeros(self.stats()["n_glyphs"] + 1, dtype=np.uint32)
        self.ctx._check(L.vgsdf_batch_segments_read(self.ctx._h, self._h, seg_off.ctypes.data, None, None, None, None))
        ns = int(seg_off[-1])
        cols = [np.zeros(ns, dtype=np.float64) for _ in range(4)]
        self.ctx._check(L.vgsdf_batch_segments_read(self.ctx._h, self._h, seg_off.ctypes.data, *[c.ctypes.data for c in cols]))
        return seg_off, np.stack(cols, axis=1) if ns else np.zeros((0, 4))

    def free(self):
        if self._h:
            load_library().vgsdf_batch_free(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass


class ResidentFont:
    """vgsdf_font: a face's outlines resident on a context's device (any context of that device may name it)."""

    def __init__(self, ctx: "SdfContext", handle):
        self.ctx, self._h = ctx, handle

    @property
    def device_bytes(self) -> int:
        return int(load_library().vgsdf_font_device_bytes(self._h)) if self._h else 0

    def free(self):
        """the caller's to time: no submission that names the font may be in flight"""
        if self._h and self.ctx._h:
            load_library().vgsdf_font_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ResidentFamily:
    """vgsdf_family: the table code point -> (font, glyph id, advance, scale, shift_x) of a font id, resident beside its fonts
    (which it does not own: they must outlive it)."""

    def __init__(self, ctx: "SdfContext", handle, fonts):
        self.ctx, self._h, self.fonts = ctx, handle, list(fonts)

    @property
    def device_bytes(self) -> int:
        return int(load_library().vgsdf_family_device_bytes(self._h)) if self._h else 0

    @property
    def plane(self) -> int:
        """vgsdf_family_plane: the plane whose low halves the family's code points are"""
        return int(load_library().vgsdf_family_plane(self._h)) if self._h else 0

    def count(self, first: int, last: int) -> int:
        """mapped code points in [first, last] (low halves, whatever the plane)"""
        return int(load_library().vgsdf_family_count(self._h, first, last))

    def free(self):
        """the caller's to time: no submission that names the family may be in flight"""
        if self._h and self.ctx._h:
            load_library().vgsdf_family_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SdfContext:
    """vgsdf_ctx: one per (thread, GPU)."""

    def __init__(self, device: int = 0):
        L = load_library()
        h = C.c_void_p()
        rc = L.vgsdf_create(device, C.byref(h))
        if rc != 0:
            raise VgsdfError(rc, (L.vgsdf_last_error(None) or b"").decode())
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            raise VgsdfError(rc, (load_library().vgsdf_last_error(self._h) or b"").decode())

    def last_error(self) -> str:
        """vgsdf_last_error: the words of this context's last failure or per-item refusal (a call that returns VGSDF_OK with a
        status that is not leaves them here)"""
        return (load_library().vgsdf_last_error(self._h) or b"").decode()

    def set_variant(self, v: int):
        self._check(load_library().vgsdf_set_variant(self._h, v))

    def add_counters(self, blocks: int, glyphs: int, pixels: int):
        load_library().vgsdf_add_counters(self._h, blocks, glyphs, pixels)

    def reset_counters(self):
        load_library().vgsdf_reset_counters(self._h)

    def render_batch(self, batch: Batch) -> np.ndarray:
        out = np.empty(batch.out_bytes, dtype=np.uint8)
        cb = batch.c_struct()
        self._check(load_library().vgsdf_render_batch(self._h, C.byref(cb), out.ctypes.data))
        return out

    def upload(self, batch: Batch) -> DeviceBatch:
        cb = batch.c_struct()
        h = C.c_void_p()
        self._check(load_library().vgsdf_batch_upload(self._h, C.byref(cb), C.byref(h)))
        self.sync()
        return DeviceBatch(self, h, batch.out_bytes)

    def outlines_prepare(self, cmd_off, cmds, scale, shift_x):
        """device front-end, step 1: outline commands -> (rects, out_bytes, n_segments)"""
        cmd_off = np.ascontiguousarray(cmd_off, dtype=np.uint32)
        cmds = np.ascontiguousarray(cmds, dtype=OUTLINE_CMD_DTYPE)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        shift_x = np.ascontiguousarray(shift_x, dtype=np.float64)
        n = len(scale)
        rects = np.zeros(n, dtype=RECT_DTYPE)
        ob, ns = C.c_uint64(0), C.c_uint64(0)
        co = _COutlines(n, cmd_off.ctypes.data, cmds.ctypes.data, scale.ctypes.data, shift_x.ctypes.data)
        self._check(load_library().vgsdf_outlines_prepare(self._h, C.byref(co), rects.ctypes.data, C.byref(ob), C.byref(ns)))
        self._fe = (n, int(ob.value), int(ns.value))
        return rects, int(ob.value), int(ns.value)

    def outlines_render_into(self, cmd_off, cmds, scale, shift_x, capacity: int, pinned: bool = True):
        """device front-end as ONE submission -> (rects, bitmaps | None, out_bytes, n_segments); bitmaps is None when
        `capacity` bytes were too few (the batch stays prepared: outlines_render() finishes it)"""
        L = load_library()
        cmd_off = np.ascontiguousarray(cmd_off, dtype=np.uint32)
        cmds = np.ascontiguousarray(cmds, dtype=OUTLINE_CMD_DTYPE)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        shift_x = np.ascontiguousarray(shift_x, dtype=np.float64)
        n = len(scale)
        rects = np.zeros(n, dtype=RECT_DTYPE)
        ob, ns, done = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        co = _COutlines(n, cmd_off.ctypes.data, cmds.ctypes.data, scale.ctypes.data, shift_x.ctypes.data)
        host = L.vgsdf_host_alloc(max(capacity, 1)) if pinned else None
        if pinned and not host:
            raise MemoryError("vgsdf_host_alloc")
        try:
            buf = (C.c_uint8 * max(capacity, 1)).from_address(host) if pinned else (C.c_uint8 * max(capacity, 1))()
            self._check(L.vgsdf_outlines_render_into(self._h, C.byref(co), rects.ctypes.data, C.addressof(buf), capacity,
                                                     C.byref(ob), C.byref(ns), C.byref(done)))
            self._fe = (n, int(ob.value), int(ns.value))
            out = np.frombuffer(buf, dtype=np.uint8, count=int(ob.value)).copy() if done.value else None
        finally:
            if pinned:
                L.vgsdf_host_free(host)
        return rects, out, int(ob.value), int(ns.value)

    def _submit(self, entry: str, co, keep: dict, capacity: int, pbf_pre=None, pbf_fix=None, fill=None, pinned=True, n=None):
        """what the outlines_submit* wrappers share: the PBF arrays attached to the C struct `co`, a page-locked output buffer
        (freed when the submit fails), and the arrays, the buffer and the glyph count kept until outlines_wait.  fill: a byte
        the buffer is filled with first; pinned=False: a pageable buffer (numpy's) instead"""
        L = load_library()
        if pbf_pre is not None:
            keep["pbf_pre"] = np.ascontiguousarray(pbf_pre, dtype=np.uint32)
            co.pbf_pre = keep["pbf_pre"].ctypes.data
        if pbf_fix is not None:
            keep["pbf_fix"] = np.ascontiguousarray(pbf_fix, dtype=np.uint8)
            co.pbf_fix = keep["pbf_fix"].ctypes.data
        if not pinned:      # numpy owns the buffer: the fifth entry of _inflight keeps it, and tells outlines_wait not to free it
            pageable = np.full(max(capacity, 1), 0 if fill is None else fill, dtype=np.uint8)
            self._check(getattr(L, entry)(self._h, C.byref(co), pageable.ctypes.data, capacity))
            self._inflight = (keep, pageable.ctypes.data, capacity, co.n_glyphs if n is None else n, pageable)
            return
        host = L.vgsdf_host_alloc(max(capacity, 1))
        if not host:
            raise MemoryError("vgsdf_host_alloc")
        if fill is not None:
            C.memset(host, fill, max(capacity, 1))
        rc = getattr(L, entry)(self._h, C.byref(co), host, capacity)
        if rc != 0:
            L.vgsdf_host_free(host)
            self._check(rc)
        self._inflight = (keep, host, capacity, co.n_glyphs if n is None else n)

    def outlines_submit(self, cmd_off, cmds, scale, shift_x, capacity: int):
        """first half of the one-submission form: everything is enqueued, nothing waited for (one per context)"""
        keep = {
            "cmd_off": np.ascontiguousarray(cmd_off, dtype=np.uint32), "cmds": np.ascontiguousarray(cmds, dtype=OUTLINE_CMD_DTYPE),
            "scale": np.ascontiguousarray(scale, dtype=np.float64), "shift": np.ascontiguousarray(shift_x, dtype=np.float64),
        }
        co = _COutlines(len(keep["scale"]), keep["cmd_off"].ctypes.data, keep["cmds"].ctypes.data, keep["scale"].ctypes.data,
                        keep["shift"].ctypes.data)
        self._submit("vgsdf_outlines_submit", co, keep, capacity)

    @staticmethod
    def pack_outlines(cmd_off, cmds):
        """28-byte command records -> (dat_off, kinds, coords) of vgsdf_outlines_packed"""
        cmds = np.ascontiguousarray(cmds, dtype=OUTLINE_CMD_DTYPE)
        kinds = cmds["kind"].astype(np.uint8)
        nf = np.select([cmds["kind"] <= 1, cmds["kind"] == 2, cmds["kind"] == 3], [2, 4, 6], 0).astype(np.int64)
        at = np.concatenate([[0], np.cumsum(nf)])
        coords = np.zeros(int(at[-1]), dtype=np.float32)
        for fields, k in ((("x", "y"), (0, 1)), (("x1", "y1", "x", "y"), (2,)), (("x1", "y1", "x2", "y2", "x", "y"), (3,))):
            sel = np.isin(cmds["kind"], k)
            for j, f in enumerate(fields):
                coords[at[:-1][sel] + j] = cmds[f][sel]
        dat_off = at[np.asarray(cmd_off, dtype=np.int64)].astype(np.uint32)
        return dat_off, kinds, coords

    def outlines_submit_packed(self, cmd_off, dat_off, kinds, coords, scale, shift_x, capacity: int, pbf_pre=None, pbf_fix=None):
        """outlines_submit for the compact upload form (vgsdf_outlines_packed); pbf_pre / pbf_fix: in-place PBF assembly"""
        keep = {
            "cmd_off": np.ascontiguousarray(cmd_off, dtype=np.uint32), "dat_off": np.ascontiguousarray(dat_off, dtype=np.uint32),
            "kinds": np.ascontiguousarray(kinds, dtype=np.uint8), "coords": np.ascontiguousarray(coords, dtype=np.float32),
            "scale": np.ascontiguousarray(scale, dtype=np.float64), "shift": np.ascontiguousarray(shift_x, dtype=np.float64),
        }
        co = _COutlinesPacked(len(keep["scale"]), keep["cmd_off"].ctypes.data, keep["dat_off"].ctypes.data, keep["kinds"].ctypes.data,
                              keep["coords"].ctypes.data, keep["scale"].ctypes.data, keep["shift"].ctypes.data)
        self._submit("vgsdf_outlines_submit_packed", co, keep, capacity, pbf_pre, pbf_fix)

    def outlines_submit_glyf(self, cmd_off, parts, glyf_bytes, scale, shift_x, capacity: int, pbf_pre=None, pbf_fix=None):
        """outlines_submit for glyphs that arrive as their `glyf` arrays (vgsdf_outlines_glyf): the device decodes them"""
        keep = {
            "cmd_off": np.ascontiguousarray(cmd_off, dtype=np.uint32), "parts": np.ascontiguousarray(parts, dtype=GLYF_PART_DTYPE),
            "bytes": np.ascontiguousarray(glyf_bytes, dtype=np.uint8),
            "scale": np.ascontiguousarray(scale, dtype=np.float64), "shift": np.ascontiguousarray(shift_x, dtype=np.float64),
        }
        co = _COutlinesGlyf(len(keep["scale"]), len(keep["parts"]), len(keep["bytes"]), keep["cmd_off"].ctypes.data, keep["parts"].ctypes.data,
                            keep["bytes"].ctypes.data, keep["scale"].ctypes.data, keep["shift"].ctypes.data)
        self._submit("vgsdf_outlines_submit_glyf", co, keep, capacity, pbf_pre, pbf_fix)

    def font_create(self, leaf_off, leaves, store) -> ResidentFont:
        """vgsdf_font_create: a face's description (vgsdf_font_desc: leaf_off[numGlyphs + 1], leaves, bytes) -> ResidentFont"""
        leaf_off = np.ascontiguousarray(leaf_off, dtype=np.uint32)
        leaves = np.ascontiguousarray(leaves, dtype=GLYF_PART_DTYPE)
        store = np.ascontiguousarray(store, dtype=np.uint8)
        d = _CFontDesc(max(len(leaf_off), 1) - 1, len(leaves), len(store), leaf_off.ctypes.data, leaves.ctypes.data, store.ctypes.data)
        h = C.c_void_p()
        self._check(load_library().vgsdf_font_create(self._h, C.byref(d), C.byref(h)))
        return ResidentFont(self, h)

    def font_create_commands(self, cmd_off, dat_off, kinds, coords) -> ResidentFont:
        """vgsdf_font_create_commands: a face's outline commands by glyph id (vgsdf_font_cmds_desc: cmd_off / dat_off[numGlyphs + 1]
        into kinds / coords, the arrays of the packed form) -> ResidentFont, named by outlines_submit_resident like any other"""
        cmd_off = np.ascontiguousarray(cmd_off, dtype=np.uint32)
        dat_off = np.ascontiguousarray(dat_off, dtype=np.uint32)
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        assert len(cmd_off) == len(dat_off) >= 1
        d = _CFontCmdsDesc(len(cmd_off) - 1, len(kinds), len(coords), cmd_off.ctypes.data, dat_off.ctypes.data, kinds.ctypes.data,
                           coords.ctypes.data)
        h = C.c_void_p()
        self._check(load_library().vgsdf_font_create_commands(self._h, C.byref(d), C.byref(h)))
        return ResidentFont(self, h)

    def font_create_charstrings(self, desc: dict, max_store_bytes=None, **override):
        """vgsdf_font_create_charstrings: a `CFF ` face's charstrings (vgsdf_font_charstrings_desc as a dict: bytes, cs_off,
        gsubr_off, lsubr_first, lsubr_off, fd_of or None — what FontManager.charstring_font_desc returns) -> the command font the
        DEVICE decodes from them.  override: raw struct fields (n_glyph_ids, n_bytes, n_gsubrs, n_fds) for descriptions that lie.
        VgsdfError with code VGSDF_E_GLYF: the device refuses the face (seac, token budget, store bounds).
        max_store_bytes (vgsdf_font_create_charstrings_within): -> (ResidentFont or None when the store would pass it, store bytes)"""
        d, keep = _CFontCharstringsDesc(), {}
        self._fill_charstrings_desc(d, keep, desc, override)
        h = C.c_void_p()
        if max_store_bytes is not None:
            want = C.c_uint64()
            self._check(load_library().vgsdf_font_create_charstrings_within(self._h, C.byref(d), int(max_store_bytes), C.byref(h), C.byref(want)))
            return (ResidentFont(self, h) if h.value else None), int(want.value)
        self._check(load_library().vgsdf_font_create_charstrings(self._h, C.byref(d), C.byref(h)))
        return ResidentFont(self, h)

    @staticmethod
    def _fill_charstrings_desc(d, keep, desc, override):
        keep.update({k: np.ascontiguousarray(desc[k], dtype=np.uint32) for k in ("cs_off", "gsubr_off", "lsubr_first", "lsubr_off")})
        keep["bytes"] = np.ascontiguousarray(desc["bytes"], dtype=np.uint8)
        fd_of = desc.get("fd_of")
        keep["fd_of"] = None if fd_of is None or len(fd_of) == 0 else np.ascontiguousarray(fd_of, dtype=np.uint8)
        d.n_glyph_ids = override.get("n_glyph_ids", len(keep["cs_off"]) - 1)
        d.n_bytes = override.get("n_bytes", len(keep["bytes"]))
        d.bytes = keep["bytes"].ctypes.data
        d.cs_off = keep["cs_off"].ctypes.data
        d.n_gsubrs = override.get("n_gsubrs", len(keep["gsubr_off"]) - 1)
        d.gsubr_off = keep["gsubr_off"].ctypes.data
        d.n_fds = override.get("n_fds", len(keep["lsubr_first"]) - 1)
        d.lsubr_first = keep["lsubr_first"].ctypes.data
        d.lsubr_off = keep["lsubr_off"].ctypes.data
        d.fd_of = None if keep["fd_of"] is None else keep["fd_of"].ctypes.data

    def font_create_charstrings2(self, desc: dict, max_store_bytes=None, **override):
        """vgsdf_font_create_charstrings2: a `CFF2` face's charstrings and blend sets (vgsdf_font_charstrings2_desc as a dict: the keys
        of font_create_charstrings plus set_ok, set_off, factors — what FontManager.charstring2_font_desc returns) -> the command
        font the DEVICE decodes from them.  override: raw struct fields (those of font_create_charstrings, n_sets, n_factors).
        Errors and max_store_bytes as font_create_charstrings."""
        d, keep = _CFontCharstrings2Desc(), {}
        self._fill_charstrings_desc(d.charstrings, keep, desc, override)
        keep["set_ok"] = np.ascontiguousarray(desc["set_ok"], dtype=np.uint8)
        keep["set_off"] = np.ascontiguousarray(desc["set_off"], dtype=np.uint32)
        keep["factors"] = np.ascontiguousarray(desc["factors"], dtype=np.float32)
        d.n_sets = override.get("n_sets", len(keep["set_ok"]))
        d.n_factors = override.get("n_factors", len(keep["factors"]))
        d.set_ok = keep["set_ok"].ctypes.data
        d.set_off = keep["set_off"].ctypes.data
        d.factors = keep["factors"].ctypes.data
        h = C.c_void_p()
        if max_store_bytes is not None:
            want = C.c_uint64()
            self._check(load_library().vgsdf_font_create_charstrings2_within(self._h, C.byref(d), int(max_store_bytes), C.byref(h), C.byref(want)))
            return (ResidentFont(self, h) if h.value else None), int(want.value)
        self._check(load_library().vgsdf_font_create_charstrings2(self._h, C.byref(d), C.byref(h)))
        return ResidentFont(self, h)

    def fonts_create_charstrings2(self, desc: dict, positions, max_store_bytes=None, **override):
        """vgsdf_fonts_create_charstrings2: ONE `CFF2` face (desc as font_create_charstrings2 takes it; its own "factors" is not
        looked at) at every position of `positions` (each the n_factors f32 factors of that position, laid out by set_off) in one
        call -> (fonts, statuses, needed), each a list per position: a ResidentFont or None; VGSDF_OK with a font, VGSDF_OK without
        one when the store would pass what the positions before it have left of max_store_bytes
        (vgsdf_fonts_create_charstrings2_within; needed: the store's bytes, 0 without a limit or for a refused position),
        VGSDF_E_GLYF for a position the device refuses.  VgsdfError: the whole call failed.
        override (for calls that lie): n_positions, the raw struct fields of font_create_charstrings2; null: the names among
        "desc", "factors", "out", "status" to pass as NULL"""
        d, keep = _CFontsCharstrings2Desc(), {}
        self._fill_charstrings_desc(d.face.charstrings, keep, desc, override)
        keep["set_ok"] = np.ascontiguousarray(desc["set_ok"], dtype=np.uint8)
        keep["set_off"] = np.ascontiguousarray(desc["set_off"], dtype=np.uint32)
        factors = np.asarray(positions, dtype=np.float32)
        factors = np.ascontiguousarray(factors.reshape(len(positions), factors.size // max(len(positions), 1)))
        null = set(override.get("null", ()))
        d.face.n_sets = override.get("n_sets", len(keep["set_ok"]))
        d.face.n_factors = override.get("n_factors", factors.shape[1] if len(positions) else len(desc["factors"]))
        d.face.set_ok = keep["set_ok"].ctypes.data
        d.face.set_off = keep["set_off"].ctypes.data
        d.face.factors = factors.ctypes.data if factors.size and "factors" not in null else None
        d.n_positions = n = int(override.get("n_positions", len(positions)))
        room = max(len(positions), n if n <= 4096 else 0, 1)
        out, status, needed = (C.c_void_p * room)(), (C.c_int * room)(), (C.c_uint64 * room)()
        args = [None if "desc" in null else C.byref(d)]
        tail = [None if "out" in null else out, None if "status" in null else status]
        L = load_library()
        try:
            if max_store_bytes is not None:
                self._check(L.vgsdf_fonts_create_charstrings2_within(self._h, *args, int(max_store_bytes), *tail, needed))
            else:
                self._check(L.vgsdf_fonts_create_charstrings2(self._h, *args, *tail))
        except VgsdfError:
            assert not any(out[i] for i in range(room)), "a failed call left a font behind"
            raise
        k = min(n, room)
        return ([ResidentFont(self, C.c_void_p(out[i])) if out[i] else None for i in range(k)], [int(status[i]) for i in range(k)],
                [int(needed[i]) for i in range(k)])

    def fonts_charstrings2_kernel_ms(self):
        """(count, emit) pass milliseconds of this context's last fonts_create_charstrings2"""
        ms = (C.c_float * 2)()
        load_library().vgsdf_fonts_charstrings2_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def font_charstrings_kernel_ms(self):
        """(count, emit) pass milliseconds of this context's last font_create_charstrings / font_create_charstrings2"""
        ms = (C.c_float * 2)()
        load_library().vgsdf_font_charstrings_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def font_commands_read(self, font: ResidentFont) -> dict:
        """vgsdf_font_commands_read (test / inspection): a command font's store as {cmd_off, records (OUTLINE_CMD_DTYPE), context}"""
        L = load_library()
        n, n_cmds = C.c_uint32(), C.c_uint32()
        self._check(L.vgsdf_font_commands_read(self._h, font._h, C.byref(n), C.byref(n_cmds), None, None, None))
        cmd_off = np.zeros(n.value + 1, dtype=np.uint32)
        records = np.zeros(n_cmds.value, dtype=OUTLINE_CMD_DTYPE)
        context = np.zeros(n_cmds.value, dtype=np.uint8)
        self._check(L.vgsdf_font_commands_read(self._h, font._h, None, None, cmd_off.ctypes.data, records.ctypes.data, context.ctypes.data))
        return {"cmd_off": cmd_off, "records": records, "context": context}

    def font_create_tables(self, desc: dict, max_store_bytes=None, **override):
        """vgsdf_font_create_tables: a `glyf` face's tables (vgsdf_font_tables_desc as a dict: loca, glyf (bytes or uint8 arrays),
        num_glyphs, loca_entries, loca_long — what FontManager.font_tables_desc returns) -> the glyf-kind font the DEVICE walks
        from them.  override: raw struct fields (n_loca_bytes, n_glyf_bytes) for descriptions that lie.
        VgsdfError with code VGSDF_E_GLYF: the device refuses the face (component budget, the bounds of the resident form).
        max_store_bytes (vgsdf_font_create_tables_within): -> (ResidentFont or None when the store would pass it, store bytes)"""
        loca, glyf = np.frombuffer(bytes(desc["loca"]), dtype=np.uint8), np.frombuffer(bytes(desc["glyf"]), dtype=np.uint8)
        d = _CFontTablesDesc(int(desc["num_glyphs"]), int(desc["loca_entries"]), int(desc["loca_long"]),
                             override.get("n_loca_bytes", len(loca)), override.get("n_glyf_bytes", len(glyf)),
                             loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)
        h = C.c_void_p()
        if max_store_bytes is not None:
            want = C.c_uint64()
            self._check(load_library().vgsdf_font_create_tables_within(self._h, C.byref(d), int(max_store_bytes), C.byref(h), C.byref(want)))
            return (ResidentFont(self, h) if h.value else None), int(want.value)
        self._check(load_library().vgsdf_font_create_tables(self._h, C.byref(d), C.byref(h)))
        return ResidentFont(self, h)

    def font_create_gvar(self, desc: dict, max_store_bytes=None, **override):
        """vgsdf_font_create_gvar: a placed `glyf` face's tables and position (vgsdf_font_gvar_desc as a dict: the keys of
        font_create_tables plus gvar (bytes) and coords (int16, one per axis) — what FontManager.gvar_font_desc returns) -> the
        command font the DEVICE builds from them.  override: raw struct fields (n_loca_bytes, n_glyf_bytes, gvar_len, n_axes) for
        descriptions that lie.  VgsdfError with code VGSDF_E_GLYF: the device refuses the face (malformed variation data,
        VGSDF_GVAR_MAX_DELTAS, the walk's and the store's bounds).
        max_store_bytes (vgsdf_font_create_gvar_within): -> (ResidentFont or None when the store would pass it, store bytes)"""
        loca, glyf = np.frombuffer(bytes(desc["loca"]), dtype=np.uint8), np.frombuffer(bytes(desc["glyf"]), dtype=np.uint8)
        gvar = np.frombuffer(bytes(desc["gvar"]), dtype=np.uint8)
        coords = np.ascontiguousarray(desc["coords"], dtype=np.int16)
        d = _CFontGvarDesc()
        d.tables = _CFontTablesDesc(int(desc["num_glyphs"]), int(desc["loca_entries"]), int(desc["loca_long"]),
                                    override.get("n_loca_bytes", len(loca)), override.get("n_glyf_bytes", len(glyf)),
                                    loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)
        d.gvar = gvar.ctypes.data if len(gvar) else None
        d.gvar_len = override.get("gvar_len", len(gvar))
        d.n_axes = override.get("n_axes", len(coords))
        d.coords = coords.ctypes.data if len(coords) else None
        h = C.c_void_p()
        if max_store_bytes is not None:
            want = C.c_uint64()
            self._check(load_library().vgsdf_font_create_gvar_within(self._h, C.byref(d), int(max_store_bytes), C.byref(h), C.byref(want)))
            return (ResidentFont(self, h) if h.value else None), int(want.value)
        self._check(load_library().vgsdf_font_create_gvar(self._h, C.byref(d), C.byref(h)))
        return ResidentFont(self, h)

    @staticmethod
    def _gvar_desc(desc: dict, keep: list, override=None):
        """vgsdf_font_gvar_desc of a dict as font_create_gvar takes it; the arrays it points to are appended to keep"""
        override = override or {}
        loca, glyf = np.frombuffer(bytes(desc["loca"]), dtype=np.uint8), np.frombuffer(bytes(desc["glyf"]), dtype=np.uint8)
        gvar = np.frombuffer(bytes(desc["gvar"]), dtype=np.uint8)
        coords = np.ascontiguousarray(desc["coords"], dtype=np.int16)
        keep += [loca, glyf, gvar, coords]
        d = _CFontGvarDesc()
        d.tables = _CFontTablesDesc(int(override.get("num_glyphs", desc["num_glyphs"])), int(override.get("loca_entries", desc["loca_entries"])),
                                    int(desc["loca_long"]), override.get("n_loca_bytes", len(loca)), override.get("n_glyf_bytes", len(glyf)),
                                    loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)
        d.gvar = gvar.ctypes.data if len(gvar) else None
        d.gvar_len = override.get("gvar_len", len(gvar))
        d.n_axes = override.get("n_axes", len(coords))
        d.coords = coords.ctypes.data if len(coords) else None
        return d

    def gvar_advance_deltas(self, desc: dict, **override):
        """vgsdf_gvar_advance_deltas: the phantom pass alone over a placed `glyf` face (desc as font_create_gvar takes it), read
        back -> (delta float32[num_glyphs], state uint8[num_glyphs]: 0 none, 1 delta, 2 malformed).  override: raw struct fields
        (num_glyphs, loca_entries, n_loca_bytes, n_glyf_bytes, gvar_len, n_axes) for descriptions that lie.  VgsdfError with code
        VGSDF_E_GLYF: a glyph id past VGSDF_GVAR_MAX_DELTAS"""
        keep = []
        d = self._gvar_desc(desc, keep, override)
        n = int(d.tables.num_glyphs)
        delta, state = np.full(max(n, 1), np.nan, np.float32), np.full(max(n, 1), 0xEE, np.uint8)
        self._check(load_library().vgsdf_gvar_advance_deltas(self._h, C.byref(d), delta.ctypes.data, state.ctypes.data))
        return delta[:n], state[:n]

    def gvar_advance_kernel_ms(self) -> float:
        """milliseconds of the phantom pass of this context's last gvar_advance_deltas / family_create_tables_gvar"""
        return float(load_library().vgsdf_gvar_advance_kernel_ms(self._h))

    def font_gvar_kernel_ms(self):
        """(count, deltas, emit) pass milliseconds of this context's last font_create_gvar"""
        ms = (C.c_float * 3)()
        load_library().vgsdf_font_gvar_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1]), float(ms[2])

    def font_read(self, font: ResidentFont) -> dict:
        """vgsdf_font_read (test / inspection): the DEVICE's copy of a glyf-kind font as {leaf_off, leaves (GLYF_PART_DTYPE), bytes},
        whichever call made it"""
        L = load_library()
        n, n_leaves, n_bytes = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(L.vgsdf_font_read(self._h, font._h, C.byref(n), C.byref(n_leaves), C.byref(n_bytes), None, None, None))
        leaf_off = np.zeros(n.value + 1, dtype=np.uint32)
        leaves = np.zeros(n_leaves.value, dtype=GLYF_PART_DTYPE)
        store = np.zeros(n_bytes.value, dtype=np.uint8)
        self._check(L.vgsdf_font_read(self._h, font._h, None, None, None, leaf_off.ctypes.data, leaves.ctypes.data, store.ctypes.data))
        return {"leaf_off": leaf_off, "leaves": leaves, "bytes": store}

    def font_tables_kernel_ms(self):
        """(count, emit + copy) milliseconds of the kernels of this context's last font_create_tables"""
        ms = (C.c_float * 2)()
        load_library().vgsdf_font_tables_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def fonts_create_tables(self, descs, max_store_bytes=None, **override):
        """vgsdf_fonts_create_tables: the glyf-kind fonts of ALL `descs` (each as font_create_tables takes it; the keys n_loca_bytes /
        n_glyf_bytes, when present, overrule the tables' lengths) built by one count and one emit launch -> a list, per face, of
        (ResidentFont or None, status, needed): status VGSDF_OK with a font, VGSDF_OK without one when the store would pass what
        the faces before it have left of max_store_bytes (vgsdf_fonts_create_tables_within; needed: its bytes, 0 without a limit),
        VGSDF_E_ARG for a bad description, VGSDF_E_GLYF for a face the device refuses.  VgsdfError: the whole call failed.
        override (for calls that lie): n_faces; null: the names among "faces", "out", "status" to pass as NULL"""
        keep = []
        arr = (_CFontTablesDesc * max(len(descs), 1))()
        for i, desc in enumerate(descs):
            loca, glyf = np.frombuffer(bytes(desc["loca"]), dtype=np.uint8), np.frombuffer(bytes(desc["glyf"]), dtype=np.uint8)
            keep.append((loca, glyf))
            arr[i] = _CFontTablesDesc(int(desc["num_glyphs"]), int(desc["loca_entries"]), int(desc["loca_long"]),
                                      int(desc.get("n_loca_bytes", len(loca))), int(desc.get("n_glyf_bytes", len(glyf))),
                                      loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)
        n = int(override.get("n_faces", len(descs)))
        null = set(override.get("null", ()))
        out = (C.c_void_p * max(len(descs), 1))()
        status = (C.c_int * max(len(descs), 1))()
        needed = (C.c_uint64 * max(len(descs), 1))()
        args = [None if "faces" in null else arr, n]
        tail = [None if "out" in null else out, None if "status" in null else status]
        L = load_library()
        try:
            if max_store_bytes is not None:
                self._check(L.vgsdf_fonts_create_tables_within(self._h, *args, int(max_store_bytes), *tail, needed))
            else:
                self._check(L.vgsdf_fonts_create_tables(self._h, *args, *tail))
        except VgsdfError:
            assert not any(out[i] for i in range(len(descs))), "a failed call left a font behind"
            raise
        return [(ResidentFont(self, C.c_void_p(out[i])) if out[i] else None, int(status[i]), int(needed[i])) for i in range(min(n, len(descs)))]

    def fonts_tables_kernel_ms(self):
        """(count, emit + copy) milliseconds of the two launches of this context's last fonts_create_tables"""
        ms = (C.c_float * 2)()
        load_library().vgsdf_fonts_tables_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def fonts_create_gvar(self, desc: dict, positions, max_store_bytes=None, **override):
        """vgsdf_fonts_create_gvar: ONE placed `glyf` face (desc as font_create_gvar takes it; its own "coords" is not looked at) at
        every position of `positions` (each n_axes normalised int16 coordinates) in one call -> (fonts, statuses, needed), each a
        list per position: a ResidentFont or None; VGSDF_OK with a font, VGSDF_OK without one when the store would pass what the
        positions before it have left of max_store_bytes (vgsdf_fonts_create_gvar_within; needed: the store's bytes, 0 without a
        limit), VGSDF_E_GLYF for a position the device refuses.  VgsdfError: the whole call failed.
        override (for calls that lie): n_positions, n_axes, n_loca_bytes, n_glyf_bytes, gvar_len; null: the names among "desc",
        "gvar", "coords", "out", "status" to pass as NULL"""
        loca, glyf = np.frombuffer(bytes(desc["loca"]), dtype=np.uint8), np.frombuffer(bytes(desc["glyf"]), dtype=np.uint8)
        gvar = np.frombuffer(bytes(desc["gvar"]), dtype=np.uint8)
        coords = np.ascontiguousarray(np.asarray(positions, dtype=np.int16).reshape(len(positions), -1 if len(positions) else 0))
        null = set(override.get("null", ()))
        d = _CFontsGvarDesc()
        d.tables = _CFontTablesDesc(int(desc["num_glyphs"]), int(desc["loca_entries"]), int(desc["loca_long"]),
                                    override.get("n_loca_bytes", len(loca)), override.get("n_glyf_bytes", len(glyf)),
                                    loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)
        d.gvar = gvar.ctypes.data if len(gvar) and "gvar" not in null else None
        d.gvar_len = override.get("gvar_len", len(gvar))
        d.n_axes = override.get("n_axes", coords.shape[1] if len(positions) else len(desc["coords"]))
        d.coords = coords.ctypes.data if coords.size and "coords" not in null else None
        d.n_positions = n = int(override.get("n_positions", len(positions)))
        room = max(len(positions), n if n <= 4096 else 0, 1)
        out, status, needed = (C.c_void_p * room)(), (C.c_int * room)(), (C.c_uint64 * room)()
        args = [None if "desc" in null else C.byref(d)]
        tail = [None if "out" in null else out, None if "status" in null else status]
        L = load_library()
        try:
            if max_store_bytes is not None:
                self._check(L.vgsdf_fonts_create_gvar_within(self._h, *args, int(max_store_bytes), *tail, needed))
            else:
                self._check(L.vgsdf_fonts_create_gvar(self._h, *args, *tail))
        except VgsdfError:
            assert not any(out[i] for i in range(room)), "a failed call left a font behind"
            raise
        k = min(n, room)
        return ([ResidentFont(self, C.c_void_p(out[i])) if out[i] else None for i in range(k)], [int(status[i]) for i in range(k)],
                [int(needed[i]) for i in range(k)])

    def fonts_gvar_kernel_ms(self):
        """(count, deltas, emit) pass milliseconds of this context's last fonts_create_gvar"""
        ms = (C.c_float * 3)()
        load_library().vgsdf_fonts_gvar_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1]), float(ms[2])

    def outlines_submit_resident_mixed(self, fonts, font_of, glyph_id, scale, shift_x, capacity: int, pbf_pre=None, pbf_fix=None, fill=None):
        """vgsdf_outlines_submit_resident_mixed: outlines_submit_resident with fonts of BOTH kinds (glyf and command fonts) in `fonts`"""
        self.outlines_submit_resident(fonts, font_of, glyph_id, scale, shift_x, capacity, pbf_pre, pbf_fix, fill,
                                      entry="vgsdf_outlines_submit_resident_mixed")

    def outlines_submit_resident(self, fonts, font_of, glyph_id, scale, shift_x, capacity: int, pbf_pre=None, pbf_fix=None, fill=None,
                                 entry="vgsdf_outlines_submit_resident"):
        """outlines_submit for glyphs named by (font, glyph id) of resident fonts (vgsdf_outlines_resident)"""
        keep = {
            "font_of": np.ascontiguousarray(font_of, dtype=np.uint16), "glyph_id": np.ascontiguousarray(glyph_id, dtype=np.uint16),
            "scale": np.ascontiguousarray(scale, dtype=np.float64), "shift": np.ascontiguousarray(shift_x, dtype=np.float64),
            "fonts": (C.c_void_p * max(len(fonts), 1))(*[f._h for f in fonts]), "font_objects": list(fonts),
        }
        n = len(keep["scale"])
        assert len(keep["font_of"]) == n and len(keep["glyph_id"]) == n
        co = _COutlinesResident(n, len(fonts), C.cast(keep["fonts"], C.c_void_p), keep["font_of"].ctypes.data, keep["glyph_id"].ctypes.data,
                                keep["scale"].ctypes.data, keep["shift"].ctypes.data)
        self._submit(entry, co, keep, capacity, pbf_pre, pbf_fix, fill=fill)

    def family_create_mixed(self, fonts, code_point, font_of, glyph_id, advance, scale, shift_x) -> ResidentFamily:
        """vgsdf_family_create_mixed: family_create over `fonts` of either kind -> a family of the third kind, mixed"""
        return self.family_create(fonts, code_point, font_of, glyph_id, advance, scale, shift_x, entry="vgsdf_family_create_mixed")

    def family_create_tables_mixed(self, fonts, faces) -> ResidentFamily:
        """vgsdf_family_create_tables_mixed: family_create_tables over `fonts` of either kind -> a mixed family"""
        return self.family_create_tables(fonts, faces, entry="vgsdf_family_create_tables_mixed")

    def family_create_at(self, fonts, code_point, font_of, glyph_id, advance, scale, shift_x, plane, mixed=False) -> ResidentFamily:
        """vgsdf_family_create_at: family_create (mixed: family_create_mixed) for the code points (plane << 16) | code_point"""
        return self.family_create(fonts, code_point, font_of, glyph_id, advance, scale, shift_x, entry="vgsdf_family_create_at",
                                  at=(int(mixed), int(plane)))

    def family_create_tables_at(self, fonts, faces, plane, mixed=False) -> ResidentFamily:
        """vgsdf_family_create_tables_at: family_create_tables (mixed: its _mixed twin) over the code points of `plane`"""
        return self.family_create_tables(fonts, faces, entry="vgsdf_family_create_tables_at", at=(int(mixed), int(plane)))

    def family_create(self, fonts, code_point, font_of, glyph_id, advance, scale, shift_x, entry="vgsdf_family_create", at=()) -> ResidentFamily:
        """vgsdf_family_create: the entries of a font id over `fonts` (ResidentFont, one kind), code points strictly ascending;
        at: (kind, plane) of the _at entry point"""
        a = [np.ascontiguousarray(code_point, dtype=np.uint16), np.ascontiguousarray(font_of, dtype=np.uint16),
             np.ascontiguousarray(glyph_id, dtype=np.uint16), np.ascontiguousarray(advance, dtype=np.uint32),
             np.ascontiguousarray(scale, dtype=np.float64), np.ascontiguousarray(shift_x, dtype=np.float64)]
        assert all(len(x) == len(a[0]) for x in a)
        handles = (C.c_void_p * max(len(fonts), 1))(*[f._h for f in fonts])
        d = _CFamilyDesc(len(fonts), C.cast(handles, C.c_void_p), len(a[0]), *[x.ctypes.data for x in a])
        h = C.c_void_p()
        self._check(getattr(load_library(), entry)(self._h, C.byref(d), *at, C.byref(h)))
        return ResidentFamily(self, h, fonts)

    def family_create_tables_var(self, fonts, faces, variation, mixed=False) -> ResidentFamily:
        """vgsdf_family_create_tables_var (mixed: its _mixed twin): family_create_tables with, per font, what
        FontManager.family_variation_desc returns: {hvar, store_off, map_off, region_scalars}, or {} / None for a static face;
        variation None: no record at all"""
        return self.family_create_tables(fonts, faces, entry="vgsdf_family_create_tables_var" + ("_mixed" if mixed else ""),
                                         variation=[None] * len(fonts) if variation is None else variation, no_records=variation is None)

    def family_create_tables_gvar(self, fonts, faces, variation, gvar, mixed=False, **override) -> ResidentFamily:
        """vgsdf_family_create_tables_gvar (mixed: its _mixed twin): family_create_tables_var with, per font, what
        FontManager.family_gvar_desc / gvar_font_desc returns (a dict as font_create_gvar takes it) or None for a face that takes
        nothing from gvar; gvar None: no array at all.  override: raw struct fields of every gvar description"""
        return self.family_create_tables(fonts, faces, entry="vgsdf_family_create_tables_gvar" + ("_mixed" if mixed else ""),
                                         variation=[None] * len(fonts) if variation is None else variation, no_records=variation is None,
                                         gvar=[None] * len(fonts) if gvar is None else gvar, no_gvar=gvar is None, gvar_override=override)

    @staticmethod
    def _face_table_records(faces, keep: list):
        """vgsdf_face_tables[len(faces)] of dicts as FontManager.family_tables_desc returns them; the arrays they point to are
        appended to keep"""
        recs = (_CFaceTables * max(len(faces), 1))()
        for r, t in zip(recs, faces):
            cmap, hmtx = np.frombuffer(bytes(t["cmap"]), dtype=np.uint8), np.frombuffer(bytes(t["hmtx"]), dtype=np.uint8)
            off = np.ascontiguousarray(t["subtable_off"], dtype=np.uint32)
            fmt = np.ascontiguousarray(t["subtable_format"], dtype=np.uint16)
            assert len(off) == len(fmt)
            keep += [cmap, hmtx, off, fmt]
            r.cmap, r.cmap_len = (cmap.ctypes.data if len(cmap) else None), len(cmap)
            r.hmtx, r.hmtx_len = (hmtx.ctypes.data if len(hmtx) else None), len(hmtx)
            r.units_per_em, r.num_glyphs, r.num_hmetrics = int(t["units_per_em"]), int(t["num_glyphs"]), int(t["num_hmetrics"])
            r.n_subtables = len(off)
            r.subtable_off, r.subtable_format = (off.ctypes.data if len(off) else None), (fmt.ctypes.data if len(fmt) else None)
        return recs

    def family_tables_census(self, faces) -> np.ndarray:
        """vgsdf_family_tables_census: uint32[136], bit b set where some face's unicode subtable lists a code point of block b
        (256 b .. 256 b + 255) that is no surrogate; faces: dicts as family_create_tables takes them (no fonts are needed)"""
        keep = []
        recs = self._face_table_records(faces, keep)
        d = _CFamilyTablesDesc(len(faces), None, C.cast(recs, C.c_void_p))
        bits = np.full(136, 0xEEEEEEEE, np.uint32)
        self._check(load_library().vgsdf_family_tables_census(self._h, C.byref(d), bits.ctypes.data))
        return bits

    def family_census_kernel_ms(self) -> float:
        return float(load_library().vgsdf_family_census_kernel_ms(self._h))

    def family_create_tables(self, fonts, faces, entry="vgsdf_family_create_tables", variation=None, no_records=False, gvar=None,
                             no_gvar=False, gvar_override=None, at=()) -> ResidentFamily:
        """vgsdf_family_create_tables: the family of `fonts` (ResidentFont, one kind, provider order) built on the device from
        `faces`, one dict per font as FontManager.family_tables_desc returns it: {cmap, hmtx (bytes or uint8 arrays),
        units_per_em, num_glyphs, num_hmetrics, subtable_off, subtable_format}"""
        assert len(fonts) == len(faces)
        keep = []
        recs = self._face_table_records(faces, keep)
        handles = (C.c_void_p * max(len(fonts), 1))(*[f._h for f in fonts])
        d = _CFamilyTablesDesc(len(fonts), C.cast(handles, C.c_void_p), C.cast(recs, C.c_void_p))
        h = C.c_void_p()
        if variation is None:
            self._check(getattr(load_library(), entry)(self._h, C.byref(d), *at, C.byref(h)))  # (at: kind and plane of the _at entry point)
            return ResidentFamily(self, h, fonts)
        assert len(variation) == len(fonts)
        vrecs = (_CFaceVariation * max(len(fonts), 1))()
        for r, v in zip(vrecs, variation):
            if not v:
                continue
            hv = np.frombuffer(bytes(v["hvar"]), dtype=np.uint8)
            sc = np.ascontiguousarray(v["region_scalars"], dtype=np.float32)
            keep += [hv, sc]
            r.hvar, r.hvar_len = (hv.ctypes.data if len(hv) else None), int(v.get("hvar_len", len(hv)))
            r.store_off, r.map_off = int(v["store_off"]), int(v["map_off"])
            r.region_scalars, r.n_regions = (sc.ctypes.data if len(sc) else None), len(sc)
        if gvar is None:
            self._check(getattr(load_library(), entry)(self._h, C.byref(d), None if no_records else C.cast(vrecs, C.c_void_p), C.byref(h)))
            return ResidentFamily(self, h, fonts)
        assert len(gvar) == len(fonts)
        gdescs = [self._gvar_desc(g, keep, gvar_override) if g else None for g in gvar]
        gptrs = (C.c_void_p * max(len(fonts), 1))(*[C.addressof(g) if g is not None else None for g in gdescs])
        self._check(getattr(load_library(), entry)(self._h, C.byref(d), None if no_records else C.cast(vrecs, C.c_void_p),
                                                   None if no_gvar else C.cast(gptrs, C.c_void_p), C.byref(h)))
        return ResidentFamily(self, h, fonts)

    @staticmethod
    def _fonts_gvar_desc(desc: dict, positions, keep: list, override=None):
        """vgsdf_fonts_gvar_desc of a dict as font_create_gvar takes it (its own "coords" is not looked at) and `positions` (each
        n_axes normalised int16 coordinates); override: n_positions, n_axes, num_glyphs, loca_entries, n_loca_bytes, n_glyf_bytes,
        gvar_len; the arrays it points to are appended to keep"""
        override = override or {}
        loca, glyf = np.frombuffer(bytes(desc["loca"]), dtype=np.uint8), np.frombuffer(bytes(desc["glyf"]), dtype=np.uint8)
        gvar = np.frombuffer(bytes(desc["gvar"]), dtype=np.uint8)
        coords = np.ascontiguousarray(np.asarray(positions, dtype=np.int16).reshape(len(positions), -1 if len(positions) else 0))
        keep += [loca, glyf, gvar, coords]
        d = _CFontsGvarDesc()
        d.tables = _CFontTablesDesc(int(override.get("num_glyphs", desc["num_glyphs"])), int(override.get("loca_entries", desc["loca_entries"])),
                                    int(desc["loca_long"]), override.get("n_loca_bytes", len(loca)), override.get("n_glyf_bytes", len(glyf)),
                                    loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)
        d.gvar = gvar.ctypes.data if len(gvar) else None
        d.gvar_len = override.get("gvar_len", len(gvar))
        d.n_axes = override.get("n_axes", coords.shape[1] if len(positions) else len(desc["coords"]))
        d.coords = coords.ctypes.data if coords.size else None
        d.n_positions = int(override.get("n_positions", len(positions)))
        return d

    def gvar_advance_deltas_batch(self, desc: dict, positions, **override):
        """vgsdf_gvar_advance_deltas_batch: the phantom pass alone over ONE placed `glyf` face (desc as font_create_gvar takes it)
        at every position of `positions` in one launch, read back -> (delta float32[n_positions, num_glyphs], state uint8[same]).
        override: as gvar_advance_deltas, and n_positions.  VgsdfError with code VGSDF_E_GLYF: a glyph id past VGSDF_GVAR_MAX_DELTAS"""
        keep = []
        d = self._fonts_gvar_desc(desc, positions, keep, override)
        n, n_pos = int(d.tables.num_glyphs), len(positions)
        delta, state = np.full(max(n * n_pos, 1), np.nan, np.float32), np.full(max(n * n_pos, 1), 0xEE, np.uint8)
        self._check(load_library().vgsdf_gvar_advance_deltas_batch(self._h, C.addressof(d), delta.ctypes.data, state.ctypes.data))
        return delta[:n * n_pos].reshape(n_pos, n), state[:n * n_pos].reshape(n_pos, n)

    def families_create_tables(self, fonts, face, variation=None, gvar=None, positions=None, mixed=False, **override):
        """vgsdf_families_create_tables (mixed: its _mixed twin): the family tables of ONE face at len(fonts) positions in one call.
        fonts: the face's ResidentFont at each position; face: one dict as FontManager.family_tables_desc returns it; variation:
        None or per position what FontManager.family_variation_desc returns (records whose "hvar" bytes are equal share one
        buffer, as the call demands); gvar: None or a dict as font_create_gvar takes it, with `positions` the coordinates of every
        position -> (families, statuses), each a list per position: a ResidentFamily or None, VGSDF_OK or VGSDF_E_ARG for a
        position whose font lacks a glyph id the face maps.  VgsdfError: the whole call failed.
        override (for calls that lie): n_positions; gvar_n_positions; null: the names among "desc", "fonts", "out", "status" to
        pass as NULL; every other key is a raw field of the gvar description (as gvar_advance_deltas_batch)"""
        keep, n_fonts = [], len(fonts)
        null = set(override.pop("null", ()))
        n = int(override.pop("n_positions", n_fonts))
        gvar_n = override.pop("gvar_n_positions", None)
        d = _CFamiliesTablesDesc()
        d.n_positions = n
        handles = (C.c_void_p * max(n_fonts, 1))(*[f._h if f is not None else None for f in fonts])
        d.fonts = None if "fonts" in null else C.cast(handles, C.c_void_p)
        t, r = face, d.tables
        cmap, hmtx = np.frombuffer(bytes(t["cmap"]), dtype=np.uint8), np.frombuffer(bytes(t["hmtx"]), dtype=np.uint8)
        off, fmt = np.ascontiguousarray(t["subtable_off"], dtype=np.uint32), np.ascontiguousarray(t["subtable_format"], dtype=np.uint16)
        assert len(off) == len(fmt)
        keep += [cmap, hmtx, off, fmt]
        r.cmap, r.cmap_len = (cmap.ctypes.data if len(cmap) else None), len(cmap)
        r.hmtx, r.hmtx_len = (hmtx.ctypes.data if len(hmtx) else None), len(hmtx)
        r.units_per_em, r.num_glyphs, r.num_hmetrics = int(t["units_per_em"]), int(t["num_glyphs"]), int(t["num_hmetrics"])
        r.n_subtables = len(off)
        r.subtable_off, r.subtable_format = (off.ctypes.data if len(off) else None), (fmt.ctypes.data if len(fmt) else None)
        if variation is not None:
            assert len(variation) == n_fonts
            vrecs, shared = (_CFaceVariation * max(n_fonts, 1))(), {}
            for rec, v in zip(vrecs, variation):
                if not v:
                    continue
                raw = bytes(v["hvar"])
                hv = shared.setdefault(raw, np.frombuffer(raw, dtype=np.uint8))
                sc = np.ascontiguousarray(v["region_scalars"], dtype=np.float32)
                keep += [hv, sc]
                rec.hvar, rec.hvar_len = (hv.ctypes.data if len(hv) else None), int(v.get("hvar_len", len(hv)))
                rec.store_off, rec.map_off = int(v["store_off"]), int(v["map_off"])
                rec.region_scalars, rec.n_regions = (sc.ctypes.data if len(sc) else None), len(sc)
            keep.append(vrecs)
            d.var = C.cast(vrecs, C.c_void_p)
        if gvar is not None:
            g = self._fonts_gvar_desc(gvar, positions if positions is not None else [], keep, override)
            if gvar_n is not None:
                g.n_positions = int(gvar_n)
            keep.append(g)
            d.gvar = C.addressof(g)
        room = max(n_fonts, n if n <= 4096 else 0, 1)
        out, status = (C.c_void_p * room)(), (C.c_int * room)()
        entry = "vgsdf_families_create_tables" + ("_mixed" if mixed else "")
        try:
            self._check(getattr(load_library(), entry)(self._h, None if "desc" in null else C.addressof(d), None if "out" in null else out,
                                                       None if "status" in null else status))
        except VgsdfError:
            assert not any(out[i] for i in range(room)), "a failed call left a family behind"
            raise
        k = min(n, n_fonts)
        return ([ResidentFamily(self, C.c_void_p(out[i]), [fonts[i]]) if out[i] else None for i in range(k)], [int(status[i]) for i in range(k)])

    def families_tables_kernel_ms(self):
        """(phantom, count, emit) pass milliseconds of this context's last families_create_tables"""
        ms = (C.c_float * 3)()
        load_library().vgsdf_families_tables_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1]), float(ms[2])

    def family_read(self, family: ResidentFamily) -> dict:
        """vgsdf_family_read: the DEVICE's copy of a family's table, whichever call made it"""
        L, n = load_library(), C.c_uint32()
        self._check(L.vgsdf_family_read(self._h, family._h, C.byref(n), *[None] * 9))
        n = n.value
        a = {"code_point": np.zeros(n, np.uint16), "font_of": np.zeros(n, np.uint16), "glyph_id": np.zeros(n, np.uint16),
             "advance": np.zeros(n, np.uint32), "scale": np.zeros(n, np.float64), "shift_x": np.zeros(n, np.float64),
             "cmd_pre": np.zeros(n + 1, np.uint32), "leaf_pre": np.zeros(n + 1, np.uint32), "pbf_fix": np.zeros(n, np.uint8)}
        self._check(L.vgsdf_family_read(self._h, family._h, None, *[v.ctypes.data for v in a.values()]))
        return a

    def family_tables_kernel_ms(self):
        """(count, emit) milliseconds of the kernels of this context's last family_create_tables"""
        ms = (C.c_float * 2)()
        load_library().vgsdf_family_tables_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def outlines_submit_ranges(self, families, family_of, first, last, capacity: int, pbf_pre=None, fill=None, pinned=True):
        """outlines_submit for code-point ranges of resident families (vgsdf_outlines_ranges): task t is the mapped code points of
        [first[t], last[t]] of families[family_of[t]]; pbf_pre (per TASK): in-place PBF assembly, the device writes the entries"""
        keep = {
            "family_of": np.ascontiguousarray(family_of, dtype=np.uint16), "first": np.ascontiguousarray(first, dtype=np.uint16),
            "last": np.ascontiguousarray(last, dtype=np.uint16),
            "families": (C.c_void_p * max(len(families), 1))(*[f._h for f in families]), "family_objects": list(families),
        }
        n_tasks = len(keep["family_of"])
        assert len(keep["first"]) == n_tasks and len(keep["last"]) == n_tasks
        co = _COutlinesRanges(n_tasks, len(families), C.cast(keep["families"], C.c_void_p), keep["family_of"].ctypes.data,
                              keep["first"].ctypes.data, keep["last"].ctypes.data)
        if pbf_pre is not None:
            keep["task_pre"] = np.ascontiguousarray(pbf_pre, dtype=np.uint32)
            assert len(keep["task_pre"]) == n_tasks
            co.pbf_pre = keep["task_pre"].ctypes.data
        n = sum(families[k].count(int(a), int(b)) for k, a, b in zip(keep["family_of"], keep["first"], keep["last"])
                if k < len(families) and a <= b)
        self._n_tasks = n_tasks
        self._submit("vgsdf_outlines_submit_ranges", co, keep, capacity, fill=fill, pinned=pinned, n=n)

    def outlines_task_extents(self) -> np.ndarray:
        """after outlines_peek / outlines_wait of a ranges submission with pbf_pre: begin[n_tasks + 1] in the arena"""
        begin = np.zeros(self._n_tasks + 1, dtype=np.uint64)
        self._check(load_library().vgsdf_outlines_task_extents(self._h, begin.ctypes.data))
        return begin

    def resident_upload_bytes(self) -> int:
        """size of the block the last resident submission of this context uploaded"""
        return int(load_library().vgsdf_outlines_resident_upload_bytes(self._h))

    def outlines_peek(self):
        """between submit and wait: the front-end's results while the raster is still running -> (rects, out_bytes, in_place)"""
        ob, ip = C.c_uint64(0), C.c_int(0)
        if getattr(self, "_inflight", None) is None:  # (the library says so)
            self._check(load_library().vgsdf_outlines_peek(self._h, None, C.byref(ob), C.byref(ip)))
        keep, host, capacity, n = self._inflight[:4]
        rects = np.zeros(n, dtype=RECT_DTYPE)
        self._check(load_library().vgsdf_outlines_peek(self._h, rects.ctypes.data, C.byref(ob), C.byref(ip)))
        return rects, int(ob.value), bool(ip.value)

    def outlines_wait(self):
        """second half -> (rects, bitmaps | None, out_bytes, n_segments)"""
        L = load_library()
        keep, host, capacity, n = self._inflight[:4]
        pageable = self._inflight[4:]           # (the buffer is numpy's: kept alive to the end of this call, not freed here)
        self._inflight = None
        try:
            rects = np.zeros(n, dtype=RECT_DTYPE)
            ob, ns, done = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
            self._check(L.vgsdf_outlines_wait(self._h, rects.ctypes.data, C.byref(ob), C.byref(ns), C.byref(done)))
            self._fe = (n, int(ob.value), int(ns.value))
            buf = (C.c_uint8 * max(capacity, 1)).from_address(host)
            out = np.frombuffer(buf, dtype=np.uint8, count=int(ob.value)).copy() if done.value else None
        finally:
            if not pageable:
                L.vgsdf_host_free(host)
        return rects, out, int(ob.value), int(ns.value)

    def outlines_pbf_positions(self) -> np.ndarray:
        """after outlines_wait on a batch submitted with pbf_pre / pbf_fix: position of every glyph's bitmap in the arena"""
        at = np.zeros(self._inflight[3] if getattr(self, "_inflight", None) else self._fe[0], dtype=np.uint64)
        self._check(load_library().vgsdf_outlines_pbf_positions(self._h, at.ctypes.data))
        return at

    def outlines_render(self) -> np.ndarray:
        """device front-end, step 2: bitmaps of the glyphs with a raster, packed in glyph order"""
        out = np.empty(self._fe[1], dtype=np.uint8)
        self._check(load_library().vgsdf_outlines_render(self._h, out.ctypes.data))
        return out

    def outlines_union(self) -> np.ndarray:
        """vgsdf_outlines_union: rule U over the prepared batch (outlines_render then renders the union) -> state u8[n]"""
        n, ob, _ = self._fe
        state = np.zeros(n, dtype=np.uint8)
        ns = C.c_uint64(0)
        self._check(load_library().vgsdf_outlines_union(self._h, state.ctypes.data, C.byref(ns)))
        if n:
            self._fe = (n, ob, int(ns.value))
        return state

    def union_kernel_ms(self):
        """(count, emit) milliseconds of the last union on this context"""
        ms = (C.c_float * 2)()
        load_library().vgsdf_union_kernel_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def outlines_segments(self):
        """the segments the device front-end produced -> (seg_off[n+1], segs[S,4])"""
        n, _, ns = self._fe
        seg_off = np.zeros(n + 1, dtype=np.uint32)
        cols = [np.zeros(ns, dtype=np.float64) for _ in range(4)]
        self._check(load_library().vgsdf_outlines_segments(self._h, seg_off.ctypes.data, *[c.ctypes.data for c in cols]))
        return seg_off, np.stack(cols, axis=1) if ns else np.zeros((0, 4))

    def sync(self):
        self._check(load_library().vgsdf_sync(self._h))

    def close(self):
        if self._h:
            load_library().vgsdf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
