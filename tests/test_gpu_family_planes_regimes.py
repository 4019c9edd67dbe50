"""Families of a PLANE built on the device (vgsdf_family_create_tables_at; csrc/family_table_kernels.hip with the plane as an
argument) against vgsdf_family_create_at of the entries the Python restatement gives for the same plane
(tests/supplementary_planes_kit.py): every hand-written table whose spans reach past U+FFFF — format 12 groups inside plane 1,
across the plane edge, across the surrogates, ending at U+10FFFF and at 0xFFFFFFFF, ids that pass 0xFFFF part way, formats 13 and
10 above the BMP, a face of format 4 alone, format 4 in front of format 12, two faces that map one code point, a glyph id past
its font in plane 1 only, entries at the first and last lane, the wave edge and the workgroup edge of the grid — for planes 0, 1
and 16 and for glyf, command and mixed families.  Both families are read back with vgsdf_family_read and compared array by array,
byte for byte.  A plane whose entries name a glyph id past its font is refused by BOTH constructors with VGSDF_E_ARG, nothing is
returned and the context builds on.  Plane 0 through the new entry points is the family the old ones make.  No tolerance appears
anywhere."""
import ctypes as C

import numpy as np
import pytest

import cmap_edge_tables as E
import family_ranges_kit as K
import mixed_kinds_kit as M
import supplementary_planes_kit as S
from test_gpu_family_tables_regimes import ARRAYS

pytestmark = pytest.mark.gpu

E_ARG = -1
KINDS = ["commands", "glyf", "mixed"]
CASES = S.edge_cases()


class PlaneKit:
    """fonts for face k of a family, of one kind or (mixed) of both in turn"""

    def __init__(self, vg, ctx, kind):
        self.ctx, self.mixed = ctx, kind == "mixed"
        if self.mixed:
            self.kit = M.MixedKit(vg, ctx)
        else:
            self.kit = K.make_kit(vg, ctx, kind)

    def fonts(self, n):
        if self.mixed:
            return self.kit.handles([(k % 2, k % 3) for k in range(n)])
        return [self.kit.kinds[k % len(self.kit.kinds)] for k in range(n)]


@pytest.fixture(scope="module", params=KINDS)
def kit(vg, request):
    ctx = vg.SdfContext(0)
    try:
        yield PlaneKit(vg, ctx, request.param)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def restated():
    """(case, plane) -> the restated entries, computed once for all kinds"""
    memo = {}

    def get(name, plane):
        if (name, plane) not in memo:
            memo[name, plane] = S.restate_plane([E.describe(f) for f in CASES[name]], plane)
        return memo[name, plane]
    return get


def same_tables(ctx, got, want, r):
    a, b = ctx.family_read(got), ctx.family_read(want)
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for k in ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "pbf_fix"):
        assert a[k].tobytes() == r[k].tobytes(), k
    assert got.device_bytes == want.device_bytes and got.plane == want.plane
    for first, last in ((0, 0xFFFF), (0, 0), (0xFFFF, 0xFFFF), (0x3F, 0x100), (0xD800, 0xDFFF)):
        assert got.count(first, last) == want.count(first, last) == int(((r["code_point"] >= first) & (r["code_point"] <= last)).sum())


def both_ways(vg, kit, name, plane, r):
    """-> (device-built, host-stated) or None when BOTH constructors refuse the plane's entries"""
    faces = CASES[name]
    descs, fonts = [E.describe(f) for f in faces], kit.fonts(len(faces))
    args = (fonts, r["code_point"], r["font_of"], r["glyph_id"], r["advance"], r["scale"], r["shift_x"])
    try:
        want = kit.ctx.family_create_at(*args, plane=plane, mixed=kit.mixed)
    except vg.VgsdfError as e:
        assert e.code == E_ARG
        with pytest.raises(vg.VgsdfError) as e2:
            kit.ctx.family_create_tables_at(fonts, descs, plane, mixed=kit.mixed)
        assert e2.value.code == E_ARG
        return None
    return kit.ctx.family_create_tables_at(fonts, descs, plane, mixed=kit.mixed), want


@pytest.mark.parametrize("plane", S.PLANES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_built_plane_equals_the_host_stated_one(vg, kit, restated, name, plane):
    r = restated(name, plane)
    pair = both_ways(vg, kit, name, plane, r)
    if pair is None:
        assert int(r["glyph_id"].max()) > E.N_IDS - 1                   # (refused for the one reason there is)
        return
    got, want = pair
    same_tables(kit.ctx, got, want, r)
    assert got.plane == plane
    if plane:
        assert ((r["pbf_fix"] & 15) == 4).all()                        # 0x08 and a three-byte varint
    got.free(), want.free()


def test_the_tables_hold_what_they_are_named_for(restated):
    """(no kernel runs) which planes have entries, which are refused, and the entries at the edges"""
    def cps(name, plane):
        return restated(name, plane)["full"].tolist()
    assert cps("f12_inside_plane_1", 0) == [] and cps("f12_inside_plane_1", 1) == list(range(0x10400, 0x1040A))
    assert cps("f12_across_the_plane_edge", 0) == list(range(0xFFF8, 0x10000)) and cps("f12_across_the_plane_edge", 1) == list(range(0x10000, 0x10008))
    assert restated("f12_across_the_plane_edge", 1)["glyph_id"].tolist() == list(range(10, 18))
    assert cps("f12_fff0_to_1000f", 0) == list(range(0xFFF0, 0x10000)) and restated("f12_fff0_to_1000f", 1)["glyph_id"].tolist() == list(range(16, 32))
    sur = cps("f13_across_the_surrogates", 0)
    assert sur == list(range(0xD7F0, 0xD800)) + list(range(0xE000, 0xE010))
    assert cps("f12_ends_at_10ffff_and_at_ffffffff", 16) == list(range(0x10FFF0, 0x110000)) and cps("f13_ends_at_ffffffff", 16)[-1] == 0x10FFFF
    assert cps("f12_id_passes_ffff_part_way", 1) == list(range(0x10000, 0x10010))      # ids 0xFFF0 .. 0xFFFF, then none
    assert cps("f4_only", 1) == [] and cps("f4_only", 16) == [] and len(cps("f4_only", 0)) == 31
    ahead = restated("f4_in_front_of_f12", 0)
    assert ahead["glyph_id"].tolist() == [4, 5] and restated("f4_in_front_of_f12", 1)["glyph_id"].tolist() == [10, 11]
    two = restated("two_faces_map_10400", 1)
    assert two["full"].tolist() == [0x103FF, 0x10400, 0x10401, 0x10402] and two["font_of"].tolist() == [1, 0, 0, 1] and two["glyph_id"].tolist() == [7, 4, 5, 10]
    assert restated("past_id_in_plane_1_only", 1)["glyph_id"].tolist() == [E.PAST] and restated("past_id_in_plane_1_only", 0)["glyph_id"].tolist() == [4, 5]
    assert cps("lane_edges", 1) == S.LANE_EDGES and cps("lane_edges", 16) == [p + 0xF0000 for p in S.LANE_EDGES] and cps("lane_edges", 0) == []
    assert cps("bmp_format6", 1) == [] and 0xFFFF in cps("bmp_format6", 0)       # a 16-bit format lists nothing above the BMP
    assert cps("bmp_format10", 1) == [0x10000] and cps("bmp_format13", 1) == list(range(0x10000, 0x20000))
    assert cps("f10_first_in_plane_1", 1) == [0x10020, 0x10021, 0x10022, 0x10023, 0x1FFFE, 0x1FFFF]
    # plane 0 of the restatement is cmap_edge_tables' own
    for name in CASES:
        a, b = restated(name, 0), E.restate([E.describe(f) for f in CASES[name]])
        assert all(a[k].tobytes() == b[k].tobytes() for k in b)


def test_plane_0_through_the_new_entry_points_is_the_old_family(vg, kit, restated):
    name = "f12_across_the_plane_edge"
    faces, r = CASES[name], restated(name, 0)
    descs, fonts = [E.describe(f) for f in faces], kit.fonts(len(faces))
    args = (fonts, r["code_point"], r["font_of"], r["glyph_id"], r["advance"], r["scale"], r["shift_x"])
    old = [kit.ctx.family_create_mixed(*args) if kit.mixed else kit.ctx.family_create(*args),
           kit.ctx.family_create_tables_mixed(fonts, descs) if kit.mixed else kit.ctx.family_create_tables(fonts, descs)]
    new = [kit.ctx.family_create_at(*args, plane=0, mixed=kit.mixed), kit.ctx.family_create_tables_at(fonts, descs, 0, mixed=kit.mixed)]
    for f in old + new:
        same_tables(kit.ctx, f, old[0], r)
        assert f.plane == 0
    for f in old + new:
        f.free()


def test_refusals_return_nothing_and_the_context_builds_on(vg, kit, restated):
    L = vg.load_library()
    name = "past_id_in_plane_1_only"
    descs, fonts = [E.describe(f) for f in CASES[name]], kit.fonts(1)
    with pytest.raises(vg.VgsdfError) as e:                                # found by the count pass of plane 1 ...
        kit.ctx.family_create_tables_at(fonts, descs, 1, mixed=kit.mixed)
    assert e.value.code == E_ARG
    r = restated(name, 0)                                                  # ... while plane 0 of the same tables builds
    pair = both_ways(vg, kit, name, 0, r)
    same_tables(kit.ctx, pair[0], pair[1], r)
    for plane in (17, 255, 0xFFFFFFFF):
        for call in (lambda p: kit.ctx.family_create_tables_at(fonts, descs, p, mixed=kit.mixed),
                     lambda p: kit.ctx.family_create_at(fonts, *[r[k] for k in ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")],
                                                        plane=p, mixed=kit.mixed)):
            with pytest.raises(vg.VgsdfError) as e:
                call(plane)
            assert e.value.code == E_ARG
    h = C.c_void_p(1)
    assert L.vgsdf_family_create_tables_at(kit.ctx._h, None, 0, 1, C.byref(h)) == E_ARG
    from versatiles_glyphs_rs_amd.device import _CFamilyTablesDesc
    keep = []                                                              # (the arrays the records point to)
    recs = kit.ctx._face_table_records(descs, keep)
    handles = (C.c_void_p * 1)(fonts[0]._h)
    d = _CFamilyTablesDesc(1, C.cast(handles, C.c_void_p), C.cast(recs, C.c_void_p))
    h = C.c_void_p()
    assert L.vgsdf_family_create_tables_at(kit.ctx._h, C.byref(d), 2, 1, C.byref(h)) == E_ARG and not h.value     # a kind that is none
    assert L.vgsdf_family_plane(None) == 0
    r1 = restated("lane_edges", 1)
    got, want = both_ways(vg, kit, "lane_edges", 1, r1)
    same_tables(kit.ctx, got, want, r1)
    for f in pair + (got, want):
        f.free()
