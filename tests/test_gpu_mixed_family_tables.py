"""Mixed families built on the device from `cmap` and `hmtx` (vgsdf_family_create_tables_mixed) over faces of BOTH kinds of
resident font: the count and emit passes (csrc/family_table_kernels.hip) take a glyph's command slots and leaves from its own
face's kind, so leaf_pre stands still over an entry of a command font and cmd_pre runs over every entry.

The tables are hand-written (tests/cmap_edge_tables.py), the fonts the synthetic ones of tests/mixed_kinds_kit.py.  The yardstick
is vgsdf_family_create_mixed of the arrays the Python restatement gives for the same descriptions; both families are read back
with vgsdf_family_read and compared array by array, byte for byte, with count() and device_bytes; the prefix sums are also held
against the fonts' own glyphs.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest

import cmap_edge_tables as E
import mixed_kinds_kit as M
from mixed_kinds_kit import COMMANDS, GLYF
from test_gpu_family_tables_regimes import assert_same_family

pytestmark = pytest.mark.gpu

CASES = E.regular_cases()
# provider lists of several faces: the cases that have them, and single-face cases of differing shapes side by side
SETS = {
    "faces_2": CASES["faces_2"],
    "faces_3": CASES["faces_3"],
    "middle_face_maps_nothing": CASES["middle_face_maps_nothing"],
    "workgroups_format12_entries_257": CASES["workgroups"] + CASES["format12"] + CASES["entries_257"],
    "two_subtables_hmtx_tail_format6_format4": CASES["two_subtables"] + CASES["hmtx_tail"] + CASES["format6"] + CASES["format4_64_segments"],
    "one_face": CASES["hmtx_all_metrics"],
    "no_entry": CASES["entries_0"] + CASES["entries_0"],
}


@pytest.fixture(scope="module")
def kit(vg):
    ctx = vg.SdfContext(0)
    try:
        yield M.MixedKit(vg, ctx)
    finally:
        ctx.close()


def font_list_of(n_faces, first):
    """face k is of kind (k + first) % 2 and the kit's font k % 3"""
    return [((k + first) % 2, k % 3) for k in range(n_faces)]


def both_ways(kit, faces, font_list):
    descs = [E.describe(f) for f in faces]
    fonts = kit.handles(font_list)
    r = E.restate(descs)
    want = kit.ctx.family_create_mixed(fonts, r["code_point"], r["font_of"], r["glyph_id"], r["advance"], r["scale"], r["shift_x"])
    got = kit.ctx.family_create_tables_mixed(fonts, descs)
    return got, want, r


def assert_prefix_sums(kit, family, r, font_list):
    """cmd_pre over every entry's slots, leaf_pre over the glyf entries' leaves and 0 for an entry of a command font"""
    t = kit.ctx.family_read(family)
    glyf_font = kit.ctx.font_read(kit.kits[GLYF].kinds[0])
    leaves = np.diff(glyf_font["leaf_off"].astype(np.int64))
    kind = np.array([k for k, _ in font_list], np.int64)[r["font_of"].astype(np.int64)] if len(r["font_of"]) else np.zeros(0, np.int64)
    slots = np.array([kit.slots(int(k), int(g)) for k, g in zip(kind, r["glyph_id"])], np.int64)
    n_leaves = np.where(kind == GLYF, leaves[np.where(kind == GLYF, r["glyph_id"].astype(np.int64), 0)], 0) if len(kind) else np.zeros(0, np.int64)
    assert np.array_equal(np.diff(t["cmd_pre"].astype(np.int64)) % (1 << 32), slots)
    assert np.array_equal(np.diff(t["leaf_pre"].astype(np.int64)) % (1 << 32), n_leaves)


@pytest.mark.parametrize("first", [GLYF, COMMANDS])
@pytest.mark.parametrize("name", sorted(SETS))
def test_device_built_mixed_table_equals_the_host_stated_one(kit, name, first):
    faces = SETS[name]
    font_list = font_list_of(len(faces), first)
    got, want, r = both_ways(kit, faces, font_list)
    assert_same_family(kit.ctx, got, want, r)
    assert_prefix_sums(kit, got, r, font_list)
    if name != "no_entry":
        ms = kit.ctx.family_tables_kernel_ms()
        assert ms[0] > 0 and ms[1] > 0
    got.free(), want.free()


def test_the_large_glyphs_of_both_kinds(kit):
    every = list(range(E.N_IDS))
    faces = [E.plain_face(range(0x100, 0x100 + E.N_IDS), gids=every[1:] + [kit.big[GLYF]]),
             E.plain_face(range(0x100 + E.N_IDS, 0x100 + 3 * E.N_IDS), gids=every[1:] + [kit.big[COMMANDS]])]
    font_list = [(GLYF, 1), (COMMANDS, 2)]
    got, want, r = both_ways(kit, faces, font_list)
    assert_same_family(kit.ctx, got, want, r)
    assert_prefix_sums(kit, got, r, font_list)
    t = kit.ctx.family_read(got)
    assert int(t["cmd_pre"][-1]) > 5000 and int(t["leaf_pre"][-1]) >= 600
    got.free(), want.free()


def test_a_glyph_id_past_its_font_is_refused_and_the_context_goes_on(vg, kit):
    good = E._several_faces(1)[0]
    for font_list, faces in (([(GLYF, 0), (COMMANDS, 0)], [good] + E.past_case()), ([(COMMANDS, 0), (GLYF, 0)], [good] + E.past_case()),
                             ([(GLYF, 0), (COMMANDS, 0)], E.past_case() + [good])):
        with pytest.raises(vg.VgsdfError) as e:
            kit.ctx.family_create_tables_mixed(kit.handles(font_list), [E.describe(f) for f in faces])
        assert e.value.code == M.E_ARG
    font_list = font_list_of(3, GLYF)
    got, want, r = both_ways(kit, CASES["faces_3"], font_list)
    assert_same_family(kit.ctx, got, want, r)
    got.free(), want.free()


def test_bad_descriptions_are_refused_on_the_host(vg, kit):
    ok = E.describe(CASES["faces_1"][0])
    fonts = kit.handles([(GLYF, 0), (COMMANDS, 0)])

    def refused(fonts, **change):
        with pytest.raises(vg.VgsdfError) as e:
            kit.ctx.family_create_tables_mixed(fonts, [dict(ok, **change)] * len(fonts))
        assert e.value.code == M.E_ARG

    refused(fonts, subtable_off=np.array([len(ok["cmap"])], np.uint32))
    refused(fonts, subtable_format=np.array([2], np.uint16))
    refused(fonts, units_per_em=15)
    refused([])
    L = vg.load_library()
    h = C.c_void_p()
    assert L.vgsdf_family_create_tables_mixed(kit.ctx._h, None, C.byref(h)) == M.E_ARG and not h.value
    assert L.vgsdf_family_create_mixed(kit.ctx._h, None, C.byref(h)) == M.E_ARG and not h.value
    # the host-stated constructor: a glyph id past its face, of either kind; font_of past n_fonts; code points not ascending
    for cp, fo, gid in (([5, 6], [0, 1], [1, kit.n_ids[COMMANDS]]), ([5, 6], [0, 1], [kit.n_ids[GLYF], 1]), ([5, 6], [0, 2], [1, 1]),
                        ([6, 6], [0, 1], [1, 1])):
        with pytest.raises(vg.VgsdfError) as e:
            kit.ctx.family_create_mixed(fonts, cp, fo, gid, [0, 0], [0.024, 0.024], [0.0, 0.0])
        assert e.value.code == M.E_ARG
    # ... and the existing constructors still refuse fonts of both kinds
    with pytest.raises(vg.VgsdfError) as e:
        kit.ctx.family_create(fonts, [5, 6], [0, 1], [1, 1], [0, 0], [0.024, 0.024], [0.0, 0.0])
    assert e.value.code == M.E_ARG
    with pytest.raises(vg.VgsdfError) as e:
        kit.ctx.family_create_tables(fonts, [ok, ok])
    assert e.value.code == M.E_ARG
    got, want, r = both_ways(kit, CASES["faces_2"], font_list_of(2, COMMANDS))     # the context is sound
    assert_same_family(kit.ctx, got, want, r)
    got.free(), want.free()


def test_ranges_submission_over_a_device_built_mixed_family(kit):
    """one submission over a device-built mixed family against submit_resident_mixed of the same glyph sequence, with and
    without pbf_pre"""
    faces = CASES["faces_3"]
    font_list = font_list_of(3, COMMANDS)
    r = E.restate([E.describe(f) for f in faces])
    fam = M.MixedFamily(kit, font_list, r["code_point"], r["font_of"], r["glyph_id"], r["advance"], r["scale"], r["shift_x"], create=False)
    fam.handle = kit.ctx.family_create_tables_mixed(fam.fonts, [E.describe(f) for f in faces])
    cp = r["code_point"]
    assert set(r["font_of"].tolist()) == {0, 1, 2}
    tasks = [(0, 0, 0xFFFF, 21), (0, int(cp[3]), int(cp[17]), 9), (0, 0x2000, 0x2FFF, 4), (0, int(cp[-2]), 0xFFFF, 0)]
    rects = M.compare_ranges(kit.ctx, [fam], tasks)
    assert len(rects) == len(cp) + 15 + 2 and int(rects["has_raster"].sum()) == len(rects)
    fam.handle.free()
