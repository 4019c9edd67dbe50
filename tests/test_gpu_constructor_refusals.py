"""Every refusal of the device-built constructors of glyf tables and gvar instances, single and batched, with the WHOLE text it
leaves in vgsdf_last_error: vgsdf_font_create_tables[_within], vgsdf_fonts_create_tables[_within], vgsdf_font_create_gvar[_within]
and vgsdf_fonts_create_gvar[_within].  The single and the batched form of a constructor share their rules (csrc/resident_glyf_tables.cpp,
csrc/resident_gvar.cpp); the regime tests of the two forms are separate files that look for a word or two of a text, so a rule that
drifted between the forms, or a text that changed, would pass them.  Here each refusal is provoked on the smallest face that shows it
and the return code, status[] / needed[], *out and the text are compared with literals.

The single calls go through ctypes as they are (the wrapper of device.py raises before *out can be seen).  In the batched forms the
refusal sits at face or position 1 of 3, and what is built around it must equal the single call's store byte for byte.  Two refusals
of the gvar batch cannot sit at one position only and are tested as the call has them (tests/test_gpu_gvar_batch_regimes.py says
why): VGSDF_GVAR_MAX_DELTAS bounds tuples x points whatever the position, so every position is refused and the text names the last;
all stores of one call have one size, so a limit one byte under two stores builds position 0 and passes 1 and 2 over.

The last case is the one face here that is not small: the smallest of tests/test_gpu_gvar_regimes.py that needs more than one slice
of the deltas pass, whose plan the single and the batched call share."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytest.importorskip("fontTools")

import composite_edge_trees as T  # noqa: E402
import gvar_instances_kit as G  # noqa: E402
import test_gpu_gvar_regimes as R  # noqa: E402  (its faces and reads; its tests are not collected from here)

pytestmark = pytest.mark.gpu

OK, E_ARG, E_GLYF = 0, -1, -4

DESCRIPTION = "more than 65535 glyphs, loca_long not 0 or 1, or more loca entries than the loca bytes hold or than num_glyphs + 1"
HEADER = ("axes not 1 .. 64, a gvar that is not version 1.0 or has another axisCount, or a header, shared tuples "
          "or offset array outside gvar_len")
COMPONENTS = "a glyph past VGSDF_GLYF_MAX_COMPONENTS"
RECORDS = "a glyph past VGSDF_GLYF_MAX_COMPONENTS, or a composite of more than 65535 component records"
DELTAS = "a glyph past VGSDF_GVAR_MAX_DELTAS"
MALFORMED = "a glyph with malformed variation data"


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


def bad_descriptions(d):
    """{case: (d changed, the table lengths to state)} of a good tables description d whose loca has num_glyphs + 1 entries"""
    assert d["loca_entries"] == d["num_glyphs"] + 1 == len(d["loca"]) // (4 if d["loca_long"] else 2)
    return {"null_table": (dict(d, loca=b""), {"n_loca_bytes": len(d["loca"])}),
            "loca_long_2": (dict(d, loca_long=2), {}),
            "more_loca_entries_than_bytes": (dict(d, loca_entries=d["loca_entries"] + 1), {}),
            "loca_entries_num_glyphs_plus_2": (dict(d, num_glyphs=d["num_glyphs"] - 1), {})}


# ---- the single calls as they are ---------------------------------------------------------------------------------------------

def _tables_struct(vg, d, keep, lengths):
    dev = importlib.import_module(vg.__name__ + ".device")
    loca, glyf = np.frombuffer(bytes(d["loca"]), dtype=np.uint8), np.frombuffer(bytes(d["glyf"]), dtype=np.uint8)
    keep += [loca, glyf]
    return dev, dev._CFontTablesDesc(int(d["num_glyphs"]), int(d["loca_entries"]), int(d["loca_long"]), lengths.get("n_loca_bytes", len(loca)),
                                     lengths.get("n_glyf_bytes", len(glyf)), loca.ctypes.data if len(loca) else None, glyf.ctypes.data if len(glyf) else None)


def single(vg, ctx, d, limit=None, **lengths):
    """vgsdf_font_create_tables / _gvar (a description with "gvar"), or their _within forms under `limit` -> (return code, *out,
    *needed or None, the context's text); a font that was built is freed"""
    keep = []
    dev, tables = _tables_struct(vg, d, keep, lengths)
    name, desc = "vgsdf_font_create_tables", tables
    if "gvar" in d:
        gvar, coords = np.frombuffer(bytes(d["gvar"]), dtype=np.uint8), np.ascontiguousarray(d["coords"], dtype=np.int16)
        name, desc = "vgsdf_font_create_gvar", dev._CFontGvarDesc(tables, gvar.ctypes.data if len(gvar) else None, lengths.get("gvar_len", len(gvar)),
                                                                  lengths.get("n_axes", len(coords)), coords.ctypes.data)
    L, out, needed = dev.load_library(), C.c_void_p(), C.c_uint64(UNTOUCHED)
    if limit is None:
        rc = getattr(L, name)(ctx._h, C.byref(desc), C.byref(out))
    else:
        rc = getattr(L, name + "_within")(ctx._h, C.byref(desc), int(limit), C.byref(out), C.byref(needed))
    text = ctx.last_error()
    if out.value:
        assert L.vgsdf_font_free(ctx._h, out) == OK
    return rc, out.value, None if limit is None else int(needed.value), text


UNTOUCHED = 12345    # what single() puts into *needed before the call


def assert_single_refuses(vg, ctx, d, code, text, needed=0, **lengths):
    """both forms refuse alike; needed: what the _within form leaves in *needed"""
    assert single(vg, ctx, d, **lengths) == (code, None, None, text)
    assert single(vg, ctx, d, limit=1 << 40, **lengths) == (code, None, needed, text)


# ---- glyf tables -----------------------------------------------------------------------------------------------------------------

def glyf_store(ctx, font):
    r = ctx.font_read(font)
    return r["leaf_off"].tobytes(), r["leaves"].tobytes(), r["bytes"].tobytes(), font.device_bytes


def glyf_faces():
    """three good faces of a few glyph ids whose stores descend in size"""
    return [T.case_tables("compose_three_levels"), T.count_font(4), T.count_font(1)]


@pytest.mark.parametrize("case", ["null_table", "loca_long_2", "more_loca_entries_than_bytes", "loca_entries_num_glyphs_plus_2"])
def test_tables_single_bad_description(vg, ctx, case):
    d, lengths = bad_descriptions(T.desc(glyf_faces()[0]))[case]
    text = "NULL argument" if case == "null_table" else DESCRIPTION      # (refused before *needed is touched, or behind it)
    assert_single_refuses(vg, ctx, d, E_ARG, "vgsdf_font_create_tables: " + text, UNTOUCHED if case == "null_table" else 0, **lengths)


def test_tables_single_component_budget(vg, ctx):
    assert_single_refuses(vg, ctx, T.desc(T.budget_font(1)), E_GLYF, "vgsdf_font_create_tables: " + COMPONENTS)


def test_tables_single_one_byte_under_the_store(vg, ctx):
    d = T.desc(glyf_faces()[0])
    rc, out, want, _ = single(vg, ctx, d, limit=0)
    assert (rc, out) == (OK, None) and want > 0
    assert single(vg, ctx, d, limit=want - 1)[:3] == (OK, None, want)
    rc, out, again, _ = single(vg, ctx, d, limit=want)
    assert rc == OK and out is not None and again == want


def tables_batch(ctx, descs, expect, needed_of, text, **kw):
    """one call; expect[i]: the status of face i; needed_of[i]: its needed[] (None: as the single call states it); faces that
    are built equal the single call's store"""
    res = ctx.fonts_create_tables(descs, **kw)
    try:
        if text is not None:
            assert ctx.last_error() == text
        assert [s for _, s, _ in res] == expect
        for i, (font, status, needed) in enumerate(res):
            if needed_of[i] is not None:
                assert needed == needed_of[i] and font is None, i
                continue
            alone, size = ctx.font_create_tables(descs[i], max_store_bytes=1 << 40)
            try:
                assert needed == (size if "max_store_bytes" in kw else 0), i
                assert font is not None and glyf_store(ctx, font) == glyf_store(ctx, alone), i
            finally:
                alone.free()
    finally:
        for font, _, _ in res:
            if font is not None:
                font.free()


@pytest.mark.parametrize("case", ["null_table", "loca_long_2", "more_loca_entries_than_bytes", "loca_entries_num_glyphs_plus_2"])
@pytest.mark.parametrize("within", [False, True])
def test_tables_batch_bad_description_at_face_1(ctx, case, within):
    a, b, c = (T.desc(t) for t in glyf_faces())
    d, lengths = bad_descriptions(b)[case]
    text = "vgsdf_fonts_create_tables: face 1: a NULL table, " + DESCRIPTION
    tables_batch(ctx, [a, dict(d, **lengths), c], [OK, E_ARG, OK], [None, 0, None], text, **({"max_store_bytes": 1 << 40} if within else {}))


@pytest.mark.parametrize("within", [False, True])
def test_tables_batch_component_budget_at_face_1(ctx, within):
    a, _, c = (T.desc(t) for t in glyf_faces())
    text = "vgsdf_fonts_create_tables: face 1: " + COMPONENTS
    tables_batch(ctx, [a, T.desc(T.budget_font(1)), c], [OK, E_GLYF, OK], [None, 0, None], text, **({"max_store_bytes": 1 << 40} if within else {}))


def test_tables_batch_one_byte_under_the_store_at_face_1(ctx):
    descs = [T.desc(t) for t in glyf_faces()]
    sizes = [ctx.font_create_tables(d, max_store_bytes=0)[1] for d in descs]
    assert sizes[2] < sizes[1]
    # face 1 is passed over, face 2 goes on with the same room
    tables_batch(ctx, descs, [OK, OK, OK], [None, sizes[1], None], None, max_store_bytes=sizes[0] + sizes[1] - 1)


# ---- gvar ------------------------------------------------------------------------------------------------------------------------

def command_store(ctx, font):
    r = ctx.font_commands_read(font)
    return r["cmd_off"].tobytes(), r["records"].tobytes(), r["context"].tobytes(), font.device_bytes


def gvar_descriptions(vg):
    """{case: (description, lengths, text behind the entry's name)} of everything refused before anything runs"""
    good, _ = R._good(vg)
    gvar = good["gvar"]
    array_end = 20 + 4 * (good["num_glyphs"] + 1)
    tables = {k: good[k] for k in ("loca", "glyf", "num_glyphs", "loca_entries", "loca_long")}
    out = {case: (dict(good, **d), lengths, "NULL argument" if case == "null_table" else DESCRIPTION)
           for case, (d, lengths) in bad_descriptions(tables).items()}
    out["version"] = (dict(good, gvar=b"\0\2" + gvar[2:]), {}, HEADER)
    out["axis_count"] = (dict(good, coords=[0, 0]), {}, HEADER)
    out["offset_array_past_gvar_len"] = (dict(good, gvar=gvar[:array_end - 1]), {}, HEADER)
    return out


GVAR_DESCRIPTIONS = ["null_table", "loca_long_2", "more_loca_entries_than_bytes", "loca_entries_num_glyphs_plus_2", "version", "axis_count",
                     "offset_array_past_gvar_len"]


def budget_gvar_face():
    """the tables of the component budget's face with a gvar that has no data for any glyph id"""
    t = T.budget_font(1)
    return dict(T.desc(t), gvar=G.gvar_table([b""] * t.num_glyphs), coords=[16384])


@pytest.mark.parametrize("case", GVAR_DESCRIPTIONS)
def test_gvar_single_bad_description(vg, ctx, case):
    d, lengths, text = gvar_descriptions(vg)[case]
    assert_single_refuses(vg, ctx, d, E_ARG, "vgsdf_font_create_gvar: " + text, UNTOUCHED if case == "null_table" else 0, **lengths)


def test_gvar_single_refusals_of_the_passes(vg, ctx):
    assert_single_refuses(vg, ctx, budget_gvar_face(), E_GLYF, "vgsdf_font_create_gvar: " + RECORDS)
    font, deltas = R._budget_face(253)
    assert deltas > R.MAX_DELTAS
    # (the deltas pass refuses behind the limit's check: the store's size is stated by then)
    d = R._described(vg, font, [16384])[0]
    rc, out, want, _ = single(vg, ctx, d, limit=0)
    assert (rc, out) == (OK, None) and want > 0
    assert_single_refuses(vg, ctx, d, E_GLYF, "vgsdf_font_create_gvar: " + DELTAS, want)
    font = G.edge_faces()["composites_malformed"][0]
    assert not all(G.restate(font, [16384])["ok"])
    d = R._described(vg, font, [16384])[0]
    rc, out, want, _ = single(vg, ctx, d, limit=0)
    assert (rc, out) == (OK, None) and want > 0
    assert_single_refuses(vg, ctx, d, E_GLYF, "vgsdf_font_create_gvar: " + MALFORMED, want)


def test_gvar_single_one_byte_under_the_store(vg, ctx):
    d, host = R._good(vg)
    want = 29 * len(host["kinds"]) + 4 * len(host["cmd_off"])
    assert single(vg, ctx, d, limit=want - 1)[:3] == (OK, None, want)
    rc, out, again, _ = single(vg, ctx, d, limit=want)
    assert rc == OK and out is not None and again == want


@pytest.mark.parametrize("case", GVAR_DESCRIPTIONS)
def test_gvar_batch_bad_description_refuses_the_call(vg, ctx, case):
    d, lengths, text = gvar_descriptions(vg)[case]
    positions = [[16384], [5000], [0]] if case != "axis_count" else [[0, 0], [1, 1], [2, 2]]
    for kw in ({}, {"max_store_bytes": 1 << 40}):
        with pytest.raises(vg.VgsdfError) as e:       # (the wrapper asserts that out[] holds no font)
            ctx.fonts_create_gvar(d, positions, **lengths, **kw)
        assert e.value.code == E_ARG and str(e.value) == f"vgsdf error {E_ARG}: vgsdf_fonts_create_gvar: {text}"
        assert ctx.last_error() == "vgsdf_fonts_create_gvar: " + text


def gvar_batch(vg, ctx, font, positions, expect, text, desc=None, **kw):
    """one call; expect[p]: OK (built, equal to the single call's store there), E_GLYF (refused), None (passed over)"""
    desc = R._described(vg, font, positions[0])[0] if desc is None else desc
    fonts, status, needed = ctx.fonts_create_gvar(desc, positions, **kw)
    try:
        if text is not None:
            assert ctx.last_error() == text
        assert status == [OK if e is None else e for e in expect]
        assert [f is not None for f in fonts] == [e == OK for e in expect]
        want = None
        for p, e in enumerate(expect):
            if e == OK:
                alone, want = ctx.font_create_gvar(dict(desc, coords=positions[p]), max_store_bytes=1 << 40)
                try:
                    assert command_store(ctx, fonts[p]) == command_store(ctx, alone), p
                finally:
                    alone.free()
        for p, e in enumerate(expect):
            assert needed[p] == (0 if e == E_GLYF or "max_store_bytes" not in kw else (needed[0] if want is None else want)), p
    finally:
        for f in fonts:
            if f is not None:
                f.free()
    return needed


@pytest.mark.parametrize("within", [False, True])
def test_gvar_batch_refusals_of_the_passes(vg, ctx, within):
    kw = {"max_store_bytes": 1 << 40} if within else {}
    three = [[16384], [5000], [0]]
    # the count pass looks at no position: all refused
    gvar_batch(vg, ctx, None, three, [E_GLYF] * 3, "vgsdf_fonts_create_gvar: " + RECORDS, desc=budget_gvar_face(), **kw)
    # tuples x points whatever the scalars: all refused, the text is the last position's
    gvar_batch(vg, ctx, R._budget_face(253)[0], three, [E_GLYF] * 3, "vgsdf_fonts_create_gvar: position 2: " + DELTAS, **kw)
    # malformed at position 1 only: 0 and 2 are built
    font = G.edge_faces()["composites_malformed"][0]
    positions = [[-8192], [16384], [0]]
    assert [all(G.restate(font, p)["ok"]) for p in positions] == [True, False, True]
    gvar_batch(vg, ctx, font, positions, [OK, E_GLYF, OK], "vgsdf_fonts_create_gvar: position 1: " + MALFORMED, **kw)


def test_gvar_batch_one_byte_under_the_store(vg, ctx):
    d, host = R._good(vg)
    want = 29 * len(host["kinds"]) + 4 * len(host["cmd_off"])
    three = [[16384], [5000], [8192]]
    assert gvar_batch(vg, ctx, None, three, [None] * 3, None, desc=d, max_store_bytes=want - 1) == [want] * 3
    assert gvar_batch(vg, ctx, None, three, [OK, None, None], None, desc=d, max_store_bytes=2 * want - 1) == [want] * 3
    # a refused position takes no room: one byte under two stores builds the first that is not refused, and only that
    font = G.edge_faces()["composites_malformed"][0]
    d, host = R._described(vg, font, [-8192])
    want = 29 * len(host["kinds"]) + 4 * len(host["cmd_off"])
    text = "vgsdf_fonts_create_gvar: position 0: " + MALFORMED
    assert gvar_batch(vg, ctx, font, [[16384], [-8192], [0]], [E_GLYF, OK, None], text, max_store_bytes=2 * want - 1) == [0, want, want]


def test_the_single_call_and_a_batch_of_one_over_several_slices(vg, ctx):
    """three slices of the deltas pass (test_gpu_gvar_regimes.py, test_glyph_ids_past_a_slice_of_the_deltas_pass): the two calls
    plan them alike and leave the same store, on a context whose scratch these very launches grow"""
    desc, _ = R._described(vg, R._sliced_face(7), [16384])
    fresh = vg.SdfContext(0)
    try:
        for c in (fresh, ctx):
            alone = c.font_create_gvar(desc)
            fonts, status, _ = c.fonts_create_gvar(desc, [[16384]])
            try:
                assert status == [OK] and fonts[0] is not None
                assert command_store(c, fonts[0]) == command_store(c, alone)
            finally:
                alone.free()
                fonts[0].free()
    finally:
        fresh.close()
