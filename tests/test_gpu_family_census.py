"""The census of a font id's cmap tables on the device (vgsdf_family_tables_census; csrc/family_census_kernels.hip): a bitmap over
the 4352 blocks of 256 code points up to U+10FFFF, a bit set exactly where some unicode subtable LISTS a code point of the block
that is no surrogate.  Census = the Python restatement of that definition (tests/supplementary_planes_kit.py), bit for bit, on
every hand-written table (spans inside a plane, across the plane edge, across the surrogates, ending at U+10FFFF and at
0xFFFFFFFF, one group over everything, single code points at both ends of a word of the bitmap, whole words, more groups than a
workgroup has lanes, a face without subtables) and on all 21 fixture fonts; on the fixtures it is a superset of the blocks the
fonts map; a block whose bit is clear builds an empty range.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest

import cmap_edge_tables as E
import family_ranges_kit as K
import supplementary_planes_kit as S
from conftest import FIRA, noto_files

pytestmark = pytest.mark.gpu

E_ARG = -1
CASES = dict(S.edge_cases(), **S.census_cases())


@pytest.fixture(scope="module")
def ctx(vg):
    c = vg.SdfContext(0)
    try:
        yield c
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_census_equals_the_restatement_on_the_edge_tables(ctx, name):
    descs = [E.describe(f) for f in CASES[name]]
    want = S.census_blocks(descs)
    bits = ctx.family_tables_census(descs)
    assert bits.dtype == np.uint32 and len(bits) == S.CENSUS_WORDS and bits.tobytes() == S.census_bits(want).tobytes()
    assert not (want & set(S.SURROGATE_BLOCKS))              # (no table here lists anything else in D800 .. DFFF)


def test_the_census_tables_hold_what_they_are_named_for(ctx):
    every = set(range(S.CENSUS_BLOCKS)) - set(S.SURROGATE_BLOCKS)
    for name in ("one_group_over_everything", "one_group_past_everything"):
        got = S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES[name]]))
        assert got == every and len(got) == 4352 - 8
    ends = S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["word_ends"]]))
    assert ends == {0, 31, 32, 4320, 4351}
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["only_surrogates"]])) == set()
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["surrogates_and_one_more"]])) == {0xD7, 0xE0}
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["f12_across_the_surrogates"]])) == {0xD7, 0xE0}
    whole = S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["whole_words"]]))
    assert whole == set(range(0x1F, 0x61)) | set(range(0x200, 0x400))
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["f12_ends_at_10ffff_and_at_ffffffff"]])) == {4351}
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["format0"]])) == {0}
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["no_subtable"]])) == set()
    assert S.blocks_of_bits(ctx.family_tables_census([E.describe(f) for f in CASES["bmp_format6"]])) == {0, 0xFF, 0x100}   # [first, first + count - 1] as listed
    assert ctx.family_census_kernel_ms() > 0
    # several faces: the union
    both = ctx.family_tables_census([E.describe(CASES["word_ends"][0]), E.describe(CASES["format0"][0]), E.describe(CASES["f12_inside_plane_1"][0])])
    assert S.blocks_of_bits(both) == ends | {0x104}


def test_census_on_the_fixtures_is_the_restatement_and_a_superset_of_what_they_map(vg, ctx):
    from oracle import oracle as O
    paths = [FIRA] + noto_files()
    assert len(paths) == 21
    mgr = vg.FontManager(False)
    supplementary = 0
    for path in paths:
        fid = mgr.add_font_with_name("F" + path.stem, [path])
        d = mgr.family_tables_desc(fid, 0)
        assert d is not None
        bits = ctx.family_tables_census([d])
        assert bits.tobytes() == S.census_bits(S.census_blocks([d])).tobytes()
        font = O.Font(path)
        mapped = {int(c) >> 8 for c in font.codepoints() if int(c) <= 0x10FFFF}
        font.close()
        assert mapped <= S.blocks_of_bits(bits)
        supplementary += sum(1 for b in mapped if b >= 256)
    assert supplementary == 5                       # U+10700, U+1DF00 | U+1E700 | U+11100 | U+11300


@pytest.mark.parametrize("kind", ["commands", "glyf"])
def test_a_clear_bit_builds_an_empty_range(vg, ctx, kind):
    kit = K.make_kit(vg, ctx, kind)
    faces = CASES["lane_edges"] + CASES["f12_across_the_plane_edge"]
    descs = [E.describe(f) for f in faces]
    blocks = S.blocks_of_bits(ctx.family_tables_census(descs))
    assert blocks == {0xFF, 0x100, 0x101, 0x1FF, 0x1000, 0x1001, 0x10FF}
    fonts = [kit.kinds[0], kit.kinds[1]]
    for plane in (0, 1, 2, 16):
        fam = ctx.family_create_tables_at(fonts, descs, plane)
        for b in range(256):
            n = fam.count(256 * b, 256 * b + 255)
            assert (n > 0) == ((plane << 8) + b in blocks)       # (these tables list nothing without a value)
        fam.free()


def test_bad_descriptions_are_refused_and_the_context_goes_on(vg, ctx):
    ok = E.describe(CASES["word_ends"][0])
    for change in (dict(subtable_off=np.array([len(ok["cmap"])], np.uint32)), dict(subtable_format=np.array([14], np.uint16)), dict(units_per_em=15)):
        with pytest.raises(vg.VgsdfError) as e:
            ctx.family_tables_census([dict(ok, **change)])
        assert e.value.code == E_ARG
    with pytest.raises(vg.VgsdfError):
        ctx.family_tables_census([])
    bits = np.zeros(136, np.uint32)
    assert vg.load_library().vgsdf_family_tables_census(ctx._h, None, bits.ctypes.data) == E_ARG
    assert S.blocks_of_bits(ctx.family_tables_census([ok])) == {0, 31, 32, 4320, 4351}
