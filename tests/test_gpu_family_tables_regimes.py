"""Family tables built on the device from `cmap` and `hmtx` (vgsdf_family_create_tables; csrc/family_table_kernels.hip) at the
edges of the lookup and of the two passes: entry counts around the wave and the workgroup, workgroups that map everything,
nothing, their first or last code point only, the surrogates and 0xFFFF, every exit of the format 4 lookup, formats 0, 6, 10, 12
and 13 at their ends, several subtables, every branch of the hmtx read, units_per_em at its bounds, the steps of pbf_fix's
varints, families of several faces, a glyph id past its font, and one ranges submission over a device-built family.

The tables are hand-written (tests/cmap_edge_tables.py), the fonts the synthetic ones of family_ranges_kit, both kinds.  The
yardstick is vgsdf_family_create of the arrays the Python restatement gives for the same descriptions (pinned to the host reader
by tests/test_family_tables_desc_host.py); both families are read back with vgsdf_family_read and compared array by array, byte
for byte, with count() and device_bytes.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest

import cmap_edge_tables as E
import family_ranges_kit as K

pytestmark = pytest.mark.gpu

KINDS = ["commands", "glyf"]
E_ARG = -1
ARRAYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "cmd_pre", "leaf_pre", "pbf_fix")


@pytest.fixture(scope="module", params=KINDS)
def kit(vg, request):
    ctx = vg.SdfContext(0)
    try:
        yield K.make_kit(vg, ctx, request.param)
    finally:
        ctx.close()


def both_ways(kit, faces):
    """-> (the device-built family, its yardstick, the restated arrays); font k % 3 of the kit stands for face k"""
    descs = [E.describe(f) for f in faces]
    fonts = [kit.kinds[k % len(kit.kinds)] for k in range(len(faces))]
    r = E.restate(descs)
    want = kit.ctx.family_create(fonts, r["code_point"], r["font_of"], r["glyph_id"], r["advance"], r["scale"], r["shift_x"])
    got = kit.ctx.family_create_tables(fonts, descs)
    return got, want, r


def assert_same_family(ctx, got, want, r):
    a, b = ctx.family_read(got), ctx.family_read(want)
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for k in ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "pbf_fix"):
        assert a[k].tobytes() == r[k].tobytes(), k                      # (the yardstick holds what it was given)
    n = len(r["code_point"])
    assert len(a["code_point"]) == n and got.device_bytes == want.device_bytes
    for first, last in ((0, 0xFFFF), (0, 0), (0xFFFF, 0xFFFF), (0x41, 0x100), (0xD800, 0xDFFF), (0x300, 0x3FF)):
        assert got.count(first, last) == want.count(first, last) == int(((r["code_point"] >= first) & (r["code_point"] <= last)).sum())


CASES = E.regular_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_built_table_equals_the_yardstick(kit, name):
    got, want, r = both_ways(kit, CASES[name])
    assert_same_family(kit.ctx, got, want, r)
    ms = kit.ctx.family_tables_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0
    got.free(), want.free()


def test_the_prefix_sums_follow_the_fonts_stores(kit):
    """cmd_pre / leaf_pre of a device-built table against the kit's own glyphs, the very large one included"""
    every = list(range(E.N_IDS))
    got, want, r = both_ways(kit, [E.plain_face(range(0x100, 0x100 + 3 * E.N_IDS), gids=every[1:] + [kit.big])])
    assert_same_family(kit.ctx, got, want, r)
    t = kit.ctx.family_read(got)
    assert kit.big in r["glyph_id"].tolist() and int(t["cmd_pre"][-1]) > 1000
    assert (int(t["leaf_pre"][-1]) > 0) == (kit.name == "glyf")
    got.free(), want.free()


def test_a_glyph_id_past_its_font_is_refused_and_the_context_goes_on(vg, kit):
    descs = [E.describe(f) for f in E.past_case()]
    with pytest.raises(vg.VgsdfError) as e:
        kit.ctx.family_create_tables([kit.kinds[0]], descs)
    assert e.value.code == E_ARG
    got, want, r = both_ways(kit, CASES["faces_2"])
    assert_same_family(kit.ctx, got, want, r)
    got.free(), want.free()


def test_bad_descriptions_are_refused_on_the_host(vg, kit):
    ok = E.describe(CASES["faces_1"][0])

    def refused(fonts, **change):
        with pytest.raises(vg.VgsdfError) as e:
            kit.ctx.family_create_tables(fonts, [dict(ok, **change)] * len(fonts))
        assert e.value.code == E_ARG

    one = [kit.kinds[0]]
    refused(one, subtable_off=np.array([len(ok["cmap"])], np.uint32))                 # at the end of the table
    refused(one, subtable_off=np.array([len(ok["cmap"]) + 7], np.uint32))             # past it
    for fmt in (2, 8, 14, 1, 0xFFFF):
        refused(one, subtable_format=np.array([fmt], np.uint16))
    refused(one, units_per_em=15)
    refused(one, units_per_em=16385)
    refused([])
    other = K.make_kit(vg, kit.ctx, "glyf" if kit.name == "commands" else "commands")
    refused([kit.kinds[0], other.kinds[0]])                                           # fonts of both kinds
    L = vg.load_library()
    h = C.c_void_p()
    assert L.vgsdf_family_create_tables(kit.ctx._h, None, C.byref(h)) == E_ARG and not h.value
    got, want, r = both_ways(kit, CASES["faces_3"])                                   # the context is sound
    assert_same_family(kit.ctx, got, want, r)
    got.free(), want.free()


def test_ranges_submission_over_a_device_built_family(kit):
    """one submission over a device-built family against submit_resident of the same glyph sequence, with and without pbf_pre"""
    faces = CASES["faces_3"]
    r = E.restate([E.describe(f) for f in faces])
    fam = K.Family(kit, [0, 1, 2], r["code_point"], r["font_of"], r["glyph_id"], r["advance"], r["scale"], r["shift_x"])
    built = kit.ctx.family_create_tables(fam.fonts, [E.describe(f) for f in faces])
    host_built, fam.handle = fam.handle, built
    cp = r["code_point"]
    tasks = [(0, 0, 0xFFFF, 21), (0, int(cp[3]), int(cp[17]), 9), (0, 0x2000, 0x2FFF, 4), (0, int(cp[-2]), 0xFFFF, 0)]
    rects = K.compare(kit.ctx, [fam], tasks)
    assert len(rects) == len(cp) + 15 + 2 and int(rects["has_raster"].sum()) == len(rects)
    built.free(), host_built.free()
