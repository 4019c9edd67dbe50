"""Supplementary planes on the host (vg_manager_set_supplementary_planes), no GPU: the Python restatement of "entries of plane p"
(tests/supplementary_planes_kit.py) against the host reader on the hand-written tables and the fixtures; the block table with the
switch off and on; the dummy PBFs of the five supplementary blocks of the 20-file Noto Sans id against the oracle's DUMMY encoding
(Font.render_glyph per code point, first provider wins, oracle.pbf_encode); and glyph shards of two and three ranks, whose files
together are the single-rank files with each supplementary file written by exactly one rank.  Every comparison is byte for byte."""
import numpy as np
import pytest

import cmap_edge_tables as E
import supplementary_planes_kit as S
from conftest import FIRA, noto_files

CASES = S.edge_cases()
# (the host reader enumerates a listed span code point by code point: the tables whose groups end at 0xFFFFFFFF are the device's)
HOST_CASES = sorted(n for n in CASES if "ffffffff" not in n)


def _manager(vg, on=True, parallel=False):
    m = vg.FontManager(parallel)
    if on:
        m.set_supplementary_planes(True)
    return m


def _noto_all(vg, on=True):
    m = _manager(vg, on)
    return m, m.add_font_with_name("Noto Sans Regular", noto_files())


def _files(vg, m, r, fid=None, starts=None):
    w = vg.DummyWriter()
    m.render_glyphs(w, r, fid, starts)
    return w.files


@pytest.mark.parametrize("name", HOST_CASES)
def test_restatement_equals_the_host_reader_on_the_edge_tables(vg, name):
    """the host's block table above U+FFFF (which block, how many code points) and, glyph by glyph, advance and id of the dummy
    renderer's PbfGlyph against the restated entries of planes 1 .. 16"""
    ttLib = pytest.importorskip("fontTools.ttLib")  # noqa: F841
    from test_family_tables_desc_host import splice
    faces = CASES[name]
    m = _manager(vg)
    for f in faces:
        fid = m.add_font_data("Edge", splice(f))
    descs = [m.family_tables_desc(fid, k) for k in range(len(faces))]
    assert all(d is not None for d in descs)
    want, entries = {}, []
    for plane in range(1, 17):
        r = S.restate_plane(descs, plane)
        for c, k, a in zip(r["full"].tolist(), r["font_of"].tolist(), r["advance"].tolist()):
            want[c & ~0xFF] = want.get(c & ~0xFF, 0) + 1
            entries.append((c, k, a))
    assert m.supplementary_blocks(fid) == want
    rd = vg.Renderer.new_dummy()
    step = max(1, len(entries) // 300)                         # (two tables map a whole plane: every 400th or so of those)
    compared = 0
    for c, k, a in entries[::step] + entries[-1:]:
        g = rd.render_glyph(m, fid, c, k)
        if g is not None:                                      # (None: a glyph the renderer skips, as in the BMP)
            assert g.id == c and g.advance == a
            compared += 1
    assert compared or not entries


def test_restatement_equals_the_host_reader_on_the_fixtures(vg, oracle):
    paths = [FIRA] + noto_files()
    total = 0
    for path in paths:
        m = _manager(vg)
        fid = m.add_font_with_name("One", [path])
        d = m.family_tables_desc(fid, 0)
        want = {}
        for plane in range(1, 17):
            for c in S.restate_plane([d], plane)["full"].tolist():
                want[c & ~0xFF] = want.get(c & ~0xFF, 0) + 1
        assert m.supplementary_blocks(fid) == want
        font = oracle.Font(path)
        assert sum(want.values()) == int((font.codepoints() > 0xFFFF).sum())
        total += sum(want.values())
    assert total == S.NOTO_CODE_POINTS


def test_switch_off_nothing_changes(vg, oracle):
    m, fid = _noto_all(vg, on=False)
    r = vg.Renderer.new_dummy()
    assert m.supplementary_blocks(fid) == {}
    with pytest.raises(RuntimeError, match="bad block start"):
        m.render_glyphs(vg.DummyWriter(), r, fid, [0x10700])
    with pytest.raises(RuntimeError):
        m.render_block(r, fid, 0x10700)
    off = _files(vg, m, r)
    assert len(off) == 256
    # on and off again: the same 256 files; on: the same 256 and five more
    m.set_supplementary_planes(True)
    on = _files(vg, m, r)
    assert len(on) == 261 and all(on[k] == v for k, v in off.items())
    m.set_supplementary_planes(False)
    assert _files(vg, m, r) == off and m.supplementary_blocks(fid) == {}
    fonts = [oracle.Font(p) for p in noto_files()]
    for start in (0, 0x0900, 0xFF00):
        assert off[f"{fid}/{start}-{start + 255}.pbf"] == oracle.render_block(fonts, fid, start, oracle.DUMMY)[0]


def test_switch_on_the_block_tables_of_the_fixtures(vg):
    m, fid = _noto_all(vg)
    blocks = m.supplementary_blocks(fid)
    assert tuple(blocks) == S.NOTO_BLOCKS and sum(blocks.values()) == S.NOTO_CODE_POINTS
    assert blocks[0x10700] + blocks[0x1DF00] == 88 and blocks[0x1E700] == 28 and blocks[0x11100] == 20 and blocks[0x11300] == 4
    assert int(m.block_counts(fid).sum()) == 6480                         # (the BMP's table is what it was)
    fira = _manager(vg)
    assert fira.supplementary_blocks(fira.add_font_with_name("Fira Sans Regular", [FIRA])) == {}
    with pytest.raises(KeyError):
        m.supplementary_blocks("no_such_font")
    r = vg.Renderer.new_dummy()
    for bad in (0x10000, 0x10800, 0x10FF00, 0x110000, 0x10701):
        with pytest.raises(RuntimeError, match="bad block start"):
            m.render_glyphs(vg.DummyWriter(), r, fid, [bad])
        with pytest.raises(RuntimeError):
            m.render_block(r, fid, bad)


@pytest.mark.parametrize("in_place", [False, True], ids=["encoded", "in_place_pbf"])
def test_dummy_pbfs_of_the_five_blocks_equal_the_oracles(vg, oracle, in_place):
    m, fid = _noto_all(vg)
    m.set_in_place_pbf(in_place)
    r = vg.Renderer.new_dummy()
    want = S.OracleFonts(oracle, noto_files())
    assert tuple(want.blocks()) == S.NOTO_BLOCKS and sum(len(v) for v in want.blocks().values()) == S.NOTO_CODE_POINTS
    files = _files(vg, m, r)
    some = _files(vg, m, r, fid, [0x1DF00, 0, 0x10700])
    for start in S.NOTO_BLOCKS:
        name = f"{fid}/{start}-{start + 255}.pbf"
        pbf = want.block_pbf(fid, start, oracle.DUMMY)
        assert files[name] == pbf and m.render_block(r, fid, start) == pbf
        if name in some:
            assert some[name] == pbf
    assert sorted(some) == sorted(f"{fid}/{s}-{s + 255}.pbf" for s in (0, 0x10700, 0x1DF00))


@pytest.mark.parametrize("world", [2, 3])
def test_shard_ranks_together_write_the_single_rank_files(vg, world):
    m, fid = _noto_all(vg, True)
    r = vg.Renderer.new_dummy()
    full = _files(vg, m, r)
    assert len(full) == 261
    owner, cost = m.shard_glyphs(fid, world)
    assert len(owner) == 65536 and len(cost) == 65536 and int((owner != 0xFF).sum()) == 6480
    parts = []
    for rank in range(world):
        m.set_glyph_shard(rank, world)
        parts.append(_files(vg, m, r))
        # a rank passes a supplementary start of another rank over, and refuses one that nobody has
        mine = _files(vg, m, r, fid, list(S.NOTO_BLOCKS))
        assert sorted(mine) == sorted(f"{fid}/{s}-{s + 255}.pbf" for s in S.NOTO_BLOCKS if s // 256 % world == rank)
    m.set_glyph_shard(0, 1)
    written = {}
    for start in S.NOTO_BLOCKS:
        name = f"{fid}/{start}-{start + 255}.pbf"
        holders = [rank for rank in range(world) if name in parts[rank]]
        assert holders == [start // 256 % world]                              # exactly once, by its rank
        written[name] = parts[holders[0]][name]
    for name in full:
        if name not in written:
            written[name] = vg.pbf_merge([p[name] for p in parts])           # the BMP: every rank's partial
    assert written == full
    assert _files(vg, m, r) == full
