"""Family tables built on the device over faces AT A POSITION (vgsdf_family_create_tables_var and its _mixed twin; the VAR
instantiation of the emit pass in csrc/family_table_kernels.hip): where the lane has a glyph's `hmtx` advance it walks the face's
HVAR — advance map, ItemVariationData row, the factors the host evaluated — and adds the offset as the host's reader does.

The faces are those of tests/variable_instances_kit.py: hand-written HVAR tables at the edges of the walk (no map, both map
formats, entry sizes 1 to 4, inner widths 1 to 16 bits, indices at and past every count, word counts 0 / some / all, a region
index past the list, rows that leave the table, advances below 0 and above 65535) and the variable Fira fixtures.  The yardstick
is vgsdf_family_create of the entries the kit restates in numpy float32; both families are read back with vgsdf_family_read
and compared array by array, byte for byte, doubles as bits.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest

pytest.importorskip("fontTools")

import variable_instances_kit as K  # noqa: E402
from conftest import FIRA, noto_files  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG = -1
ARRAYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "cmd_pre", "leaf_pre", "pbf_fix")


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


class Provider:
    """one file of a family: its manager (which owns the bytes the descriptions point into), its device font, its descriptions"""

    def __init__(self, vg, ctx, font, coords=None, glyf=False):
        self.font, self.coords = font, coords
        self.mgr = vg.FontManager(False)
        self.fid = self.mgr.add_font_data("P", font) if coords is None else self.mgr.add_font_instance_normalized("P", font, coords)
        if glyf:
            d = self.mgr.resident_font_desc(self.fid)
            self.store = ctx.font_create(d["leaf_off"], d["leaves"], d["bytes"])
        else:
            d = self.mgr.command_font_desc(self.fid)
            self.store = ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"])
        self.tables = self.mgr.family_tables_desc(self.fid, 0)
        self.variation = self.mgr.family_variation_desc(self.fid, 0)
        if self.tables is None:     # an HVAR the description refuses: cmap and hmtx as the file added plainly states them
            plain = vg.FontManager(False)
            self.tables = plain.family_tables_desc(plain.add_font_data("P", font), 0)

    def raw_variation(self):
        """the record written from the kit's own reading of the file (also for an HVAR the façade's description refuses)"""
        hvar = K._table(self.font, "HVAR")
        store, amap, regions = K.hvar_parts(hvar)
        return {"hvar": hvar, "store_off": store, "map_off": amap, "region_scalars": K.region_scalars(regions, self.coords)}


def assert_same(ctx, got, want, entries):
    a, b = ctx.family_read(got), ctx.family_read(want)
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for k in entries:
        assert a[k].tobytes() == entries[k].tobytes(), k
    assert got.device_bytes == want.device_bytes and got.count(0, 0xFFFF) == len(entries["code_point"])


def both_ways(ctx, providers, mixed=False, variation=None):
    fonts = [p.store for p in providers]
    entries = K.family_entries([(p.font, p.coords) for p in providers])
    make = ctx.family_create_mixed if mixed else ctx.family_create
    want = make(fonts, *[entries[k] for k in ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")])
    var = [p.variation for p in providers] if variation is None else variation
    got = ctx.family_create_tables_var(fonts, [p.tables for p in providers], var, mixed=mixed)
    return got, want, entries


EDGE = K.hvar_edge_faces()


@pytest.mark.parametrize("case", sorted(EDGE))
def test_edge_hvar_tables_at_three_positions(vg, ctx, case):
    font, refused, desc_refused = EDGE[case]
    for coords in K.EDGE_POSITIONS:
        if refused:                                                  # no face: the record goes to the C ABI as the kit reads it
            hvar = K._table(font, "HVAR")
            store, amap, regions = K.hvar_parts(hvar)
            p = Provider(vg, ctx, font)
            rec = {"hvar": hvar, "store_off": store, "map_off": amap, "region_scalars": K.region_scalars(regions, coords)}
            with pytest.raises(vg.VgsdfError) as e:
                ctx.family_create_tables_var([p.store], [p.tables], [rec])
            assert e.value.code == E_ARG
            continue
        p = Provider(vg, ctx, font, coords)
        assert (p.variation is None) == desc_refused
        raw = p.raw_variation()
        if not desc_refused:
            assert p.variation["hvar"] == raw["hvar"] and (p.variation["store_off"], p.variation["map_off"]) == (raw["store_off"], raw["map_off"])
            assert p.variation["region_scalars"].tobytes() == raw["region_scalars"].tobytes()
        got, want, entries = both_ways(ctx, [p], variation=[raw])
        assert_same(ctx, got, want, entries)
        ms = ctx.family_tables_kernel_ms()
        assert ms[0] > 0 and ms[1] > 0
        got.free(), want.free()
        if case in ("no_map", "map1_size3_bits16", "words_all") and coords[0] > 0:     # (the edge tables do move the advances)
            static = K.family_entries([(font, None)])
            assert static["shift_x"].tobytes() != entries["shift_x"].tobytes()


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 0, 2)])
def test_a_family_of_a_static_face_and_two_instances_of_one_file(vg, ctx, order):
    fira1 = K.variable_fira(120)
    # (the static face is the file itself added plainly: a CFF2 face at its default position, without a record)
    ps = [Provider(vg, ctx, K.variable_fira(40)), Provider(vg, ctx, fira1, [8192]), Provider(vg, ctx, fira1, [16384])]
    ps = [ps[i] for i in order]
    assert [bool(p.variation) for p in ps] == [bool(p.coords) for p in ps]
    got, want, entries = both_ways(ctx, ps)
    assert_same(ctx, got, want, entries)
    # the two instances map the same code points, the first one wins; the static face maps a third of them
    assert set(entries["font_of"].tolist()) == ({0, 1} if order[0] == 0 else {0})
    got.free(), want.free()


def test_two_axes_with_avar(vg, ctx):
    font = K.variable_fira(120, two_axes=True, avar={"wght": {-1.0: -1.0, 0.0: 0.0, 0.5: 0.25, 1.0: 1.0}})
    p = Provider(vg, ctx, font, K.coords_of(font, K.EXACT_TWO_AXES))
    assert p.coords == [4096, 8192] and len(p.variation["region_scalars"]) >= 2
    got, want, entries = both_ways(ctx, [p])
    assert_same(ctx, got, want, entries)
    got.free(), want.free()


@pytest.mark.parametrize("glyf_first", [True, False])
def test_the_mixed_twin_with_a_glyf_font_beside_an_instance(vg, ctx, glyf_first):
    # (a glyf face that maps other code points than the instance does, so that both provide entries in either order)
    armenian = next(p for p in noto_files() if "Armenian" in p.name).read_bytes()
    ps = [Provider(vg, ctx, armenian, glyf=True), Provider(vg, ctx, K.variable_fira(120), [8192])]
    ps = ps if glyf_first else ps[::-1]
    got, want, entries = both_ways(ctx, ps, mixed=True)
    assert_same(ctx, got, want, entries)
    assert set(entries["font_of"].tolist()) == {0, 1}
    t = ctx.family_read(got)
    assert int(t["leaf_pre"][-1]) > 0 and int(t["cmd_pre"][-1]) > int(t["leaf_pre"][-1])
    got.free(), want.free()


def test_records_the_host_must_refuse(vg, ctx):
    p = Provider(vg, ctx, K.variable_fira(120), [8192])
    ok = p.variation
    n = len(ok["hvar"])

    def refused(**change):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.family_create_tables_var([p.store], [p.tables], [dict(ok, **change)])
        assert e.value.code == E_ARG

    refused(store_off=n - 7)                                              # the store's header leaves the table
    refused(store_off=n + 100)
    refused(map_off=n)
    refused(map_off=n + 1)
    for bad in (np.nan, np.inf, -np.inf):
        sc = ok["region_scalars"].copy()
        sc[-1] = bad
        refused(region_scalars=sc)
    hv = bytearray(ok["hvar"])
    hv[ok["store_off"] + 1] = 2                                           # a store of format 2
    refused(hvar=bytes(hv))
    # pointers beside lengths, and the out handle stays NULL
    from versatiles_glyphs_rs_amd.device import _CFaceTables, _CFaceVariation, _CFamilyTablesDesc
    L = vg.load_library()
    t = p.tables
    cmap, hmtx = np.frombuffer(t["cmap"], np.uint8), np.frombuffer(t["hmtx"], np.uint8)
    off, fmt = np.ascontiguousarray(t["subtable_off"], np.uint32), np.ascontiguousarray(t["subtable_format"], np.uint16)
    rec = _CFaceTables(cmap.ctypes.data, len(cmap), hmtx.ctypes.data, len(hmtx), t["units_per_em"], t["num_glyphs"], t["num_hmetrics"], len(off),
                       off.ctypes.data, fmt.ctypes.data)
    handles = (C.c_void_p * 1)(p.store._h)
    d = _CFamilyTablesDesc(1, C.cast(handles, C.c_void_p), C.cast(C.pointer(rec), C.c_void_p))
    for var in (_CFaceVariation(None, 40, 20, 0, None, 0), _CFaceVariation(None, 0, 0, 0, None, 3)):
        h = C.c_void_p()
        assert L.vgsdf_family_create_tables_var(ctx._h, C.byref(d), C.byref(var), C.byref(h)) == E_ARG and not h.value
    # the context is sound: a plain family, and the instance's own
    plain = Provider(vg, ctx, FIRA.read_bytes())
    a = ctx.family_create_tables([plain.store], [plain.tables])
    e = K.family_entries([(plain.font, None)])
    b = ctx.family_create([plain.store], *[e[k] for k in ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")])
    assert_same(ctx, a, b, e)
    a.free(), b.free()
    got, want, entries = both_ways(ctx, [p])
    assert_same(ctx, got, want, entries)
    got.free(), want.free()


def test_without_any_record_the_call_is_the_plain_one(vg, ctx):
    ps = [Provider(vg, ctx, FIRA.read_bytes()), Provider(vg, ctx, K.variable_fira(40))]
    fonts, tables = [p.store for p in ps], [p.tables for p in ps]
    plain = ctx.family_create_tables(fonts, tables)
    for variation in (None, [None, None], [{}, {}]):
        got = ctx.family_create_tables_var(fonts, tables, variation)
        a, b = ctx.family_read(got), ctx.family_read(plain)
        for k in ARRAYS:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert got.device_bytes == plain.device_bytes
        got.free()
    plain.free()
