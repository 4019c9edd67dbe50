"""A kit (no tests) for vgsdf_fonts_create_charstrings2, one CFF2 face at many positions in one device build: the positions a test
sends, the comparison of every store of the batched call with the single call's and with the strict interpreter's
(tests/charstring2_edge_programs.py), and hand-written programs whose CONTROL FLOW depends on the position — a `callsubr` /
`callgsubr` whose index is the result of a `blend`, a `blend` whose count is — so that two positions of one glyph deliver different
numbers of commands, one position fails where its neighbours go on, or one position alone passes the token budget.

The position-dependent faces have ONE blend set of ONE region, region 1 of the kit's variation store (peak at the axis' maximum):
a position is one factor f, which the host reader takes from the normalised `wght` coordinate.  They select no set, so set 0 it is.
"""
import numpy as np

import charstring2_edge_programs as K2
from charstring2_edge_programs import (MAX_TOKENS, NOTDEF, START, Face, alt_sets, budget_faces, cff2_table, chunk_face, enc,  # noqa: F401
                                       expected_commands, interpret, shared_face, sized_face, vals)

VGSDF_OK, VGSDF_E_ARG, VGSDF_E_GLYF = 0, -1, -4
SHIFTS = (0, 3, 5, 1, 7, 2, 4, 6)


def positions_of(desc, n, twice=True):
    """n factor arrays for `desc`: its own (the default position) and alt_sets at several shifts, neighbours unlike; from three
    positions on the last repeats the second (the same position given twice: two fonts)"""
    base = [np.asarray(desc["factors"], np.float32)] + [alt_sets(desc, s)["factors"] for s in SHIFTS]
    ps = [base[i % len(base)] for i in range(n)]
    if twice and n >= 3:
        ps[-1] = ps[1]
    return ps


def store_bytes_of(cmds):
    """what a command store of these commands occupies: 29 bytes per command, 4 per glyph id and 4"""
    return 29 * len(cmds["kinds"]) + 4 * len(cmds["cmd_off"])


def read_store(ctx, font):
    r = ctx.font_commands_read(font)
    return r["cmd_off"].tobytes(), r["records"].tobytes(), r["context"].tobytes(), font.device_bytes


class Yardsticks:
    """per description: position (the factors' bytes) -> (the single call's store, the interpreter's store, the interpreter's
    commands and ends), each made once and shared"""

    def __init__(self, ctx, desc):
        self.ctx, self.desc, self.made = ctx, desc, {}

    def at(self, factors):
        key = np.asarray(factors, np.float32).tobytes()
        if key not in self.made:
            d = dict(self.desc, factors=np.asarray(factors, np.float32))
            want, ends = expected_commands(d)
            a = self.ctx.font_create_charstrings2(d)
            b = self.ctx.font_create_commands(want["cmd_off"], want["dat_off"], want["kinds"], want["coords"])
            try:
                self.made[key] = (read_store(self.ctx, a), read_store(self.ctx, b), want, ends)
            finally:
                a.free()
                b.free()
        return self.made[key]


def assert_batch_equals_single_and_interpreter(ctx, desc, positions, yardsticks=None):
    """every position built, its store byte for byte the single call's at that position's factors and the one
    vgsdf_font_create_commands makes of the interpreter's commands -> [(commands, ends)] per position"""
    y = yardsticks or Yardsticks(ctx, desc)
    fonts, status, needed = ctx.fonts_create_charstrings2(desc, positions)
    try:
        assert status == [VGSDF_OK] * len(positions) and all(f is not None for f in fonts)
        out = []
        for p, factors in enumerate(positions):
            single, kit, want, ends = y.at(factors)
            got = read_store(ctx, fonts[p])
            assert got[0] == want["cmd_off"].tobytes(), p
            assert got == single, p
            assert got == kit, p
            out.append((want, ends))
        return out
    finally:
        for f in fonts:
            if f is not None:
                f.free()


# ---- programs whose control flow depends on the position ---------------------------------------------------------------------

def _index(i):
    """the operand that calls subroutine i of a set of fewer than 1240"""
    return i - 107


LINE = enc(5, "hlineto")
POSITION_DEPENDENT = ("blended_callsubr", "blended_blend_count", "blended_callgsubr_by_halves")


def position_dependent_face():
    """callsubr f: local subroutine 0 at f = 0 (one line), 1 at f = 1 (three), none in between (the index is no integer: the glyph
    fails there, its move stays).  blend count 1 + f: one value at f < 1 (three operands left: three lines), two at f = 1 (two).
    callgsubr 2 f: global 0, 1, 2 at f = 0, 0.5, 1 (one, two, three lines), a failure anywhere else.  Plain glyphs between them."""
    lsubrs = [enc(7, "hlineto"), enc(7, "hlineto", 8, "vlineto", 9, "hlineto")]
    gsubrs = [enc(3, 4, "rlineto"), enc(3, 4, "rlineto", 5, 6, "rlineto"), enc(3, 4, "rlineto", 5, 6, "rlineto", 7, 8, "rlineto")]
    glyphs = [(".notdef", NOTDEF), ("plain_a", START + LINE),
              ("blended_callsubr", START + enc(_index(0), 1, 1, "blend", "callsubr") + LINE),
              ("plain_b", START + enc(1, 2, 3, "hlineto")),
              ("blended_blend_count", START + enc(10, 20, 30, 40, 1, 1, 1, "blend", "blend", "hlineto")),
              ("blended_callgsubr_by_halves", START + enc(_index(0), 2, 1, "blend", "callgsubr") + LINE),
              ("plain_c", START + LINE)]
    return Face("position_dependent", glyphs, gsubrs, lsubrs, sets=[[1]])


# the lines each program delivers at f = 0, 0.5, 1 and at 0.3 (None: the glyph fails at its call)
LINES_AT = {"blended_callsubr": {0.0: 2, 0.5: None, 1.0: 4, 0.3: None}, "blended_blend_count": {0.0: 3, 0.5: 3, 1.0: 2, 0.3: 3},
            "blended_callgsubr_by_halves": {0.0: 2, 0.5: 3, 1.0: 4, 0.3: None}}


def budget_by_position_face():
    """budget_faces' nest of subroutines behind a call whose index is blended: local subroutine 9 (one token) at f = 0, 10 (two
    tokens) at f = 1.  The glyph executes exactly MAX_TOKENS tokens at f = 0 and one more at f = 1; anywhere between the index is
    no integer and the glyph fails at once.  A small glyph beside it."""
    t = [1]
    for _ in range(8):
        t.append(4 * (2 + t[-1]))
    subrs = [enc("hstem")] + [K2._call("callsubr", k - 1) * 4 for k in range(1, 9)] + [enc("hstem"), enc("hstem") * 2]
    head = enc(_index(9), 1, 1, "blend", "callsubr")       # five tokens, and the subroutine's
    left = MAX_TOKENS - 2 - 4 - 6
    body = b""
    for k in range(8, -1, -1):
        c, left = divmod(left, 2 + t[k])
        body += K2._call("callsubr", k) * c
    at = head + enc("hstem") * left + enc(0, "hmoveto") + body + enc(1, "hlineto", 1, "vlineto")
    return Face("budget_by_position", [(".notdef", NOTDEF), ("small", START + LINE), ("at_or_over", at)], [], subrs, sets=[[1]])


def window_face():
    """the kit's programs with 47 / 48 / 49 / 512 / 513 / 514 operands and with blends across slot 48 of the operand stack"""
    loc, glo = K2._shared_sets()
    picked = [(n, cs) for n, cs in K2._programs()
              if n.startswith(("stack_", "blend_values", "blend_all_above", "blend_count_on", "blend_count_below", "blend_below_after",
                               "blend_deep_then", "blend_64_regions_astride", "blend_fills_the_stack"))]
    assert len(picked) >= 15
    return Face("window", [(".notdef", NOTDEF)] + picked, glo, loc)


def launch_edge_face(n, deep):
    """chunk_face(n) with the glyph ids of `deep` filling the whole operand stack (507 operands and a blend of one value)"""
    face = chunk_face(n)
    for g in deep:
        face.glyphs[g] = (f"deep{g}", START + enc(*vals(507, g)) + K2.blend([g % 100], 4, g) + enc("hlineto"))
    return face


# ---- CFF2 files with named instances -----------------------------------------------------------------------------------------

# nine named weights, nine font ids; 525, 650 and 900 are positions the independent yardstick is valid at
NINE_WEIGHTS = [dict(subfamily=s, ps=None, location={"wght": w})
                for s, w in (("Thin", 400), ("Light", 450), ("Medium", 525), ("Semi Bold", 650), ("Bold", 700), ("Extra Bold", 800),
                             ("Black", 900), ("Extra Light", 425), ("Regular", 475))]
_FILES = {}


def instance_files():
    """name -> (font bytes, records) of the variable CFF2 Fira fixtures with instance records: built once"""
    if not _FILES:
        import named_instances_kit as N
        import variable_instances_kit as V
        _FILES["one_axis"] = (N.with_instances(V.variable_fira(120), NINE_WEIGHTS, room_for_ps=False), NINE_WEIGHTS)
        _FILES["two_axes"] = (N.with_instances(V.variable_fira(120, two_axes=True), N.TWO_AXES, room_for_ps=False), N.TWO_AXES)
        _FILES["merged_ids"] = (N.with_instances(V.variable_fira(120), N.ONE_AXIS), N.ONE_AXIS)    # two pairs of records share an id
    return _FILES
