"""A kit (no tests): hand-written CFF2 charstring programs at the edges of the interpreter's CFF2 rules, their descriptions
(vgsdf_font_charstrings2_desc as a dict of numpy arrays, built directly), the `CFF2` tables that hold them, and a strict sequential
interpreter that says what every program delivers for a given array of blend factors.

The interpreter is written from the CFF2 mode of csrc/host/cff.cpp (CharStringRun with cff2 == true): no width operand, 513
operands, `return` and `endchar` fail the glyph, a mask past the end ends the stream, a glyph ends with its data and its last
contour stays open, `vsindex` once and before any `blend`, `blend` with one f32 product and one f32 sum per delta, value n - 1
first and each value's last delta first.  The blend sets are an ARGUMENT: the description carries the reader's (the default
position), a test may pass any others.

The `CFF2` tables are written here byte by byte (header, Top DICT, INDEXes with 32-bit counts, one Font DICT, ItemVariationStore
over one axis with two regions: region 0 has its peak at 0 — factor 1 at the default position — region 1 peaks at the axis'
maximum — factor 0) and put into an OpenType shell made with fontTools' FontBuilder.  A set is a list of region indices, or
MISSING (an ItemVariationData offset past the store: the set is not usable); a set of more than 64 regions is not usable either.
"""
import io
import struct
from dataclasses import dataclass, field

import numpy as np

import charstring_edge_programs as K
from charstring_edge_programs import C, L, M, Z, bias, num  # noqa: F401

MAX_OPERANDS2, WINDOW, MAX_REGIONS, MAX_DEPTH, MAX_TOKENS = 513, 48, 64, K.MAX_DEPTH, K.MAX_TOKENS   # charstring_limits.h
MISSING = "missing"
_OP2 = {"vsindex": b"\x0f", "blend": b"\x10"}


def enc(*items):
    """K.enc with the two operators of CFF2"""
    return K.enc(*[_OP2.get(it, it) if isinstance(it, str) else it for it in items])


# ---- the interpreter ---------------------------------------------------------------------------------------------------------

class _Stop(Exception):
    pass


def blend_sets(desc):
    return {k: desc[k] for k in ("set_ok", "set_off", "factors")}


def interpret(desc, gid, sets=None, budget=MAX_TOKENS, trace=None):
    """glyph id `gid` of a CFF2 description under the blend sets `sets` ({set_ok, set_off, factors}; None: the description's).
    trace: called as trace(op, data, pos, end, stack, depth, st) for every token about to be executed, pos behind its first byte
    (and once more, with op = (12, second byte), for an escaped operator); st["scalars"] are the selected set's factors"""
    sets = blend_sets(desc) if sets is None else sets
    set_ok, set_off, factors = sets["set_ok"], sets["set_off"], np.asarray(sets["factors"], np.float32)
    data = desc["bytes"].tobytes()
    cs_off, gs_off, ls_off = desc["cs_off"], desc["gsubr_off"], desc["lsubr_off"]
    n_local, n_global = len(ls_off) - 1, len(gs_off) - 1
    f32 = np.float32
    out = K.Outcome()
    stack = []
    st = {"x": f32(0), "y": f32(0), "has_move": False, "first_move": True, "stems": 0, "scalars": None, "vsindex": False, "blend": False}

    def stop(why):
        out.end = why
        raise _Stop()

    def need(ok):
        if not ok:
            stop("fail")

    def emit(kind, *v):
        out.kinds.append(kind)
        out.coords.extend(v)

    def select(index):
        if index >= len(set_ok) or not set_ok[index]:
            return False
        st["scalars"] = factors[int(set_off[index]):int(set_off[index + 1])]
        return True

    def curve_rel(i):
        x1, y1 = st["x"] + stack[i], st["y"] + stack[i + 1]
        x2, y2 = x1 + stack[i + 2], y1 + stack[i + 3]
        st["x"], st["y"] = x2 + stack[i + 4], y2 + stack[i + 5]
        emit(C, x1, y1, x2, y2, st["x"], st["y"])

    def run(pos, end, depth):
        while pos < end:
            out.tokens += 1
            if out.tokens > budget:
                stop("budget")
            op = data[pos]
            pos += 1
            if trace is not None:
                trace(op, data, pos, end, stack, depth, st)
            if op >= 32 or op == 28:
                if op == 28:
                    need(end - pos >= 2)
                    v = f32(struct.unpack(">h", data[pos:pos + 2])[0])
                    pos += 2
                elif op <= 246:
                    v = f32(op - 139)
                elif op <= 250:
                    need(end - pos >= 1)
                    v = f32((op - 247) * 256 + data[pos] + 108)
                    pos += 1
                elif op <= 254:
                    need(end - pos >= 1)
                    v = f32(-(op - 251) * 256 - data[pos] - 108)
                    pos += 1
                else:
                    need(end - pos >= 4)
                    v = f32(struct.unpack(">i", data[pos:pos + 4])[0]) / f32(65536.0)
                    pos += 4
                need(len(stack) < MAX_OPERANDS2)
                stack.append(v)
                continue
            sp = len(stack)
            if op in (1, 3, 18, 23):
                st["stems"] += sp >> 1             # (no width: an odd operand is simply left over)
                stack.clear()
            elif op in (19, 20):
                n = sp
                stack.clear()
                if n & 1:
                    n -= 1
                st["stems"] += n >> 1
                pos = min(pos + ((st["stems"] + 7) >> 3), end)     # past the end: the stream ends
            elif op in (21, 22, 4):
                hx, hy = op != 4, op != 22
                need(sp == hx + hy)
                if st["first_move"]:
                    st["first_move"] = False
                else:
                    emit(Z)
                st["has_move"] = True
                i = 0
                if hx:
                    st["x"] = st["x"] + stack[i]
                    i += 1
                if hy:
                    st["y"] = st["y"] + stack[i]
                emit(M, st["x"], st["y"])
                stack.clear()
            elif op == 5:
                need(st["has_move"] and not (sp & 1))
                for i in range(0, sp, 2):
                    st["x"], st["y"] = st["x"] + stack[i], st["y"] + stack[i + 1]
                    emit(L, st["x"], st["y"])
                stack.clear()
            elif op in (6, 7):
                need(st["has_move"] and sp > 0)
                horizontal = op == 6
                for i in range(sp):
                    if horizontal:
                        st["x"] = st["x"] + stack[i]
                    else:
                        st["y"] = st["y"] + stack[i]
                    horizontal = not horizontal
                    emit(L, st["x"], st["y"])
                stack.clear()
            elif op == 8:
                need(st["has_move"] and sp % 6 == 0)
                for i in range(0, sp, 6):
                    curve_rel(i)
                stack.clear()
            elif op == 24:
                need(st["has_move"] and sp >= 8 and (sp - 2) % 6 == 0)
                for i in range(0, sp - 2, 6):
                    curve_rel(i)
                st["x"], st["y"] = st["x"] + stack[sp - 2], st["y"] + stack[sp - 1]
                emit(L, st["x"], st["y"])
                stack.clear()
            elif op == 25:
                need(st["has_move"] and sp >= 8 and not ((sp - 6) & 1))
                for i in range(0, sp - 6, 2):
                    st["x"], st["y"] = st["x"] + stack[i], st["y"] + stack[i + 1]
                    emit(L, st["x"], st["y"])
                curve_rel(sp - 6)
                stack.clear()
            elif op in (26, 27):
                need(st["has_move"])
                i = 0
                if sp & 1:
                    if op == 26:
                        st["x"] = st["x"] + stack[0]
                    else:
                        st["y"] = st["y"] + stack[0]
                    i = 1
                need((sp - i) % 4 == 0)
                for i in range(i, sp, 4):
                    if op == 26:
                        x1, y1 = st["x"], st["y"] + stack[i]
                        x2, y2 = x1 + stack[i + 1], y1 + stack[i + 2]
                        st["x"], st["y"] = x2, y2 + stack[i + 3]
                    else:
                        x1, y1 = st["x"] + stack[i], st["y"]
                        x2, y2 = x1 + stack[i + 1], y1 + stack[i + 2]
                        st["x"], st["y"] = x2 + stack[i + 3], y2
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                stack.clear()
            elif op in (30, 31):
                need(st["has_move"] and sp >= 4)
                horizontal = op == 31
                i = 0
                while i < sp:
                    left = sp - i
                    need(left >= 4)
                    last = stack[i + 4] if left == 5 else f32(0)
                    if horizontal:
                        x1, y1 = st["x"] + stack[i], st["y"]
                        x2, y2 = x1 + stack[i + 1], y1 + stack[i + 2]
                        st["y"] = y2 + stack[i + 3]
                        st["x"] = x2 + last
                    else:
                        x1, y1 = st["x"], st["y"] + stack[i]
                        x2, y2 = x1 + stack[i + 1], y1 + stack[i + 2]
                        st["x"] = x2 + stack[i + 3]
                        st["y"] = y2 + last
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                    i += 5 if left == 5 else 4
                    horizontal = not horizontal
                stack.clear()
            elif op in (10, 29):
                need(sp > 0 and depth < MAX_DEPTH)
                n = n_global if op == 29 else n_local
                fidx = stack.pop()
                need(np.isfinite(fidx) and float(fidx) == int(fidx))
                idx = int(fidx) + bias(n)
                need(0 <= idx < n)
                off = gs_off if op == 29 else ls_off
                run(int(off[idx]), int(off[idx + 1]), depth + 1)
            elif op == 15:                         # vsindex
                need(not st["blend"] and not st["vsindex"] and sp == 1)
                v = stack[0]
                need(v >= 0 and v <= 65535)
                need(select(int(v)))
                st["vsindex"] = True
                stack.clear()
            elif op == 16:                         # blend
                need(sp > 0)
                st["blend"] = True
                fn = stack.pop()
                need(fn >= 0 and fn <= 65535)
                n, scalars = int(fn), st["scalars"]
                k = len(scalars)
                need(len(stack) >= n * (k + 1))
                start = len(stack) - n * (k + 1)
                for i in range(n - 1, -1, -1):
                    for j in range(k):
                        delta = stack.pop()
                        stack[start + i] = f32(stack[start + i] + f32(delta * scalars[k - j - 1]))
            elif op == 12:
                need(pos < end)
                op2 = data[pos]
                pos += 1
                if trace is not None:
                    trace((12, op2), data, pos, end, stack, depth, st)
                need(st["has_move"])
                if op2 == 35:
                    need(sp == 13)
                    curve_rel(0)
                    curve_rel(6)
                elif op2 == 34:
                    need(sp == 7)
                    y0 = st["y"]
                    x1, y1 = st["x"] + stack[0], st["y"]
                    x2, y2 = x1 + stack[1], y1 + stack[2]
                    st["x"], st["y"] = x2 + stack[3], y2
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                    x1, y1 = st["x"] + stack[4], st["y"]
                    x2, y2 = x1 + stack[5], y0
                    st["x"], st["y"] = x2 + stack[6], y0
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                elif op2 == 36:
                    need(sp == 9)
                    y0 = st["y"]
                    x1, y1 = st["x"] + stack[0], st["y"] + stack[1]
                    x2, y2 = x1 + stack[2], y1 + stack[3]
                    st["x"], st["y"] = x2 + stack[4], y2
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                    x1, y1 = st["x"] + stack[5], st["y"]
                    x2, y2 = x1 + stack[6], y1 + stack[7]
                    st["x"], st["y"] = x2 + stack[8], y0
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                elif op2 == 37:
                    need(sp == 11)
                    x0, y0 = st["x"], st["y"]
                    curve_rel(0)
                    x1, y1 = st["x"] + stack[6], st["y"] + stack[7]
                    x2, y2 = x1 + stack[8], y1 + stack[9]
                    if abs(x2 - x0) > abs(y2 - y0):
                        st["x"], st["y"] = x2 + stack[10], y0
                    else:
                        st["x"], st["y"] = x0, y2 + stack[10]
                    emit(C, x1, y1, x2, y2, st["x"], st["y"])
                else:
                    stop("fail")
                stack.clear()
            else:
                stop("fail")              # 0, 2, 9, 13, 17, and 11 (return), 14 (endchar): not operators of CFF2

    try:
        with np.errstate(all="ignore"):
            if not select(0):             # set 0 is loaded before the first operator
                stop("fail")
            run(int(cs_off[gid]), int(cs_off[gid + 1]), 0)
        out.end = "end"
    except _Stop:
        pass
    return out


def expected_commands(desc, sets=None, budget=MAX_TOKENS):
    """the face's command description by the interpreter, and every glyph id's end state"""
    n = len(desc["cs_off"]) - 1
    cmd_off, dat_off, kinds, coords, ends = [0], [0], [], [], []
    for g in range(n):
        o = interpret(desc, g, sets, budget)
        kinds += o.kinds
        coords += o.coords
        cmd_off.append(len(kinds))
        dat_off.append(len(coords))
        ends.append(o.end)
    return {"cmd_off": np.array(cmd_off, np.uint32), "dat_off": np.array(dat_off, np.uint32), "kinds": np.array(kinds, np.uint8),
            "coords": np.array(coords, np.float32)}, ends


ALT = [0.3, -0.75, float(np.float32(1.0) / np.float32(3.0)), 1e-3, 1.5, -2.0, 0.0, 1.0, 7.0625]


def alt_sets(desc, shift=0):
    """the description's sets with factors no default position produces (0.3, -0.75, 1/3 as f32, 1e-3, ...), cycled"""
    n = len(desc["factors"])
    return {"set_ok": desc["set_ok"], "set_off": desc["set_off"],
            "factors": np.array([ALT[(i + shift) % len(ALT)] for i in range(n)], np.float32)}


# ---- `CFF2` tables by hand ---------------------------------------------------------------------------------------------------

def _index2(items):
    if not items:
        return struct.pack(">I", 0)
    offs = [1]
    for it in items:
        offs.append(offs[-1] + len(it))
    off_size = 1 if offs[-1] < 1 << 8 else 2 if offs[-1] < 1 << 16 else 3 if offs[-1] < 1 << 24 else 4
    return struct.pack(">IB", len(items), off_size) + b"".join(o.to_bytes(off_size, "big") for o in offs) + b"".join(items)


def _int5(v):
    return b"\x1d" + struct.pack(">i", v)


REGION_FACTOR = (1.0, 0.0)        # of regions 0 and 1 at the default position


def _vstore(sets):
    """u16 length | ItemVariationStore: one axis, region 0 = (0, 0, 0), region 1 = (0, 1, 1)"""
    regions = struct.pack(">HH", 1, 2) + struct.pack(">hhh", 0, 0, 0) + struct.pack(">hhh", 0, 16384, 16384)
    head_len = 8 + 4 * len(sets)
    body, offsets = regions, []
    for s in sets:
        if isinstance(s, str):
            offsets.append(0x00FFFF00)
            continue
        offsets.append(head_len + len(body))
        body += struct.pack(">HHH", 0, 0, len(s)) + b"".join(struct.pack(">H", r) for r in s)
    store = struct.pack(">HIH", 1, head_len, len(sets)) + b"".join(struct.pack(">I", o) for o in offsets) + body
    return struct.pack(">H", len(store)) + store


def cff2_table(charstrings, gsubrs, lsubrs, sets):
    top_len = 6 + 7 + 6
    head = b"\x02\x00\x05" + struct.pack(">H", top_len)
    gs = _index2(list(gsubrs))
    cs_at = len(head) + top_len + len(gs)
    cs = _index2(list(charstrings))
    fd_at = cs_at + len(cs)
    fd = _index2([b"\0" * 11])
    priv_at = fd_at + len(fd)
    priv = _int5(6) + b"\x13"                       # Subrs right behind the Private DICT
    fd = _index2([_int5(len(priv)) + _int5(priv_at) + b"\x12"])
    ls = _index2(list(lsubrs))
    vs_at = priv_at + len(priv) + len(ls)
    top = _int5(cs_at) + b"\x11" + _int5(fd_at) + b"\x0c\x24" + _int5(vs_at) + b"\x18"
    assert len(top) == top_len
    return head + top + gs + cs + fd + priv + ls + _vstore(sets)


_SHELLS = {}


def _shell(n_glyphs):
    """an OpenType font of n_glyphs glyph ids around a `CFF2` table, with an `fvar` of one axis (built once per count)"""
    if n_glyphs not in _SHELLS:
        from fontTools.fontBuilder import FontBuilder
        from fontTools.misc.psCharStrings import T2CharString
        names = [".notdef"] + [f"g{i}" for i in range(1, n_glyphs)]
        fb = FontBuilder(1000, isTTF=False)
        fb.setupGlyphOrder(names)
        fb.setupCharacterMap({0x100 + i: names[i] for i in range(1, min(n_glyphs, 0xFE00))})
        fb.setupNameTable({"familyName": "Synth Edge2", "styleName": "Regular"})
        fb.setupFvar([("wght", 400, 400, 900, "Weight")], [])
        fb.setupCFF2({g: T2CharString(program=[0, "hmoveto"]) for g in names}, regions=[{"wght": (0, 1, 1)}])
        fb.setupHorizontalMetrics({g: (600, 0) for g in names})
        fb.setupHorizontalHeader(ascent=935, descent=-265)
        fb.setupOS2()
        fb.setupPost()
        buf = io.BytesIO()
        fb.save(buf)
        _SHELLS[n_glyphs] = buf.getvalue()
    return _SHELLS[n_glyphs]


def otf(cff2, n_glyphs):
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    font = TTFont(io.BytesIO(_shell(n_glyphs)), recalcBBoxes=False, recalcTimestamp=False)
    raw = DefaultTable("CFF2")
    raw.data = cff2
    font["CFF2"] = raw
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


# sets of the faces below: k = 4 (factors 0 0 0 1 at the default position), k = 2 (1 0), k = 0, k = 1 (1), k = 64, and two that
# are not usable (no such subtable; 65 regions)
SETS = [[1, 1, 1, 0], [0, 1], [], [0], [0, 1] * 32, MISSING, [0, 1] * 32 + [0]]
K4, K2, K0, K1, K64, UNUSABLE, TOO_MANY, PAST = 0, 1, 2, 3, 4, 5, 6, 7
REGIONS_OF = {K4: 4, K2: 2, K0: 0, K1: 1, K64: 64}


@dataclass
class Face:
    name: str
    glyphs: list                  # (name, charstring bytes)
    gsubrs: list = field(default_factory=list)
    lsubrs: list = field(default_factory=list)
    sets: list = field(default_factory=lambda: list(SETS))
    refusal: str = ""

    def font(self):
        return otf(cff2_table([g for _, g in self.glyphs], self.gsubrs, self.lsubrs, self.sets), len(self.glyphs))

    def desc(self):
        """the description as the host states it: bodies in INDEX order (charstrings, global, local), the sets' default factors"""
        blob, offs = b"", {}
        for key, items in (("cs_off", [g for _, g in self.glyphs]), ("gsubr_off", self.gsubrs)):
            o = [len(blob)]
            for it in items:
                blob += it
                o.append(len(blob))
            offs[key] = np.array(o, np.uint32)
        lo = [len(blob)]
        for it in self.lsubrs:
            blob += it
            lo.append(len(blob))
        blob += b"\0" * (-len(blob) % 4)
        ok, off, fac = [], [0], []
        for s in self.sets:
            usable = not isinstance(s, str) and len(s) <= MAX_REGIONS
            ok.append(1 if usable else 0)
            if usable:
                fac += [REGION_FACTOR[r] for r in s]
            off.append(len(fac))
        return {"bytes": np.frombuffer(blob, np.uint8).copy(), **offs, "lsubr_first": np.array([0, len(lo) - 1], np.uint32),
                "lsubr_off": np.array(lo, np.uint32), "fd_of": None, "set_ok": np.array(ok, np.uint8),
                "set_off": np.array(off, np.uint32), "factors": np.array(fac, np.float32)}


# ---- the programs ------------------------------------------------------------------------------------------------------------

NOTDEF = enc(0, "hmoveto")
START = enc(100, 100, "rmoveto")


def vals(n, seed=0):
    return [((i + seed) * 7) % 23 - 11 for i in range(n)]


def blend(values, k, seed=0):
    """the operands of one blend over k regions and the operator: values, k deltas per value, the count"""
    n = len(values)
    deltas = [((i + seed) * 5) % 19 - 9 for i in range(n * k)]
    return enc(*values, *deltas, n, "blend")


def select(s):
    return enc(s, "vsindex") if s else b""


# call chain: level j is subroutine 10 + j of the local set for odd j, of the global set for even j; level 10 blends two values
# (set 0: four regions) and draws them
_LVL = {j: ("callsubr" if j % 2 else "callgsubr") for j in range(1, 12)}


def _call(kind, index):
    return enc(index - 107, kind)


def _shared_sets():
    loc, glo = [b""] * 22, [b""] * 22
    loc[0] = enc(10, 20, "rlineto")
    loc[1] = blend([30], 4) + enc(0, "rlineto")               # a blend whose operands are the subroutine's own
    loc[2] = enc(1, "blend")                                  # ... and one whose operands are the caller's
    loc[3] = enc(1, 2, 3, 4, "hstemhm", "hintmask")           # a mask past the end of the subroutine: the stream ends, the caller goes on
    loc[4] = enc("return")
    loc[5] = enc("endchar")
    glo[0] = enc(-5, 40, "rlineto")
    for j in range(1, 11):
        body = blend([3, 4], 4, seed=j) + enc("rlineto") if j == 10 else _call(_LVL[j + 1], 10 + j + 1)
        (loc if j % 2 else glo)[10 + j] = body
    loc[21] = _call(_LVL[1], 11)                              # one level in front of the chain: its level 10 would be the 11th call
    return loc, glo


_OPERATORS = [("hstem", 2), ("vstem", 2), ("hstemhm", 2), ("vstemhm", 2), ("hintmask", 2), ("cntrmask", 2), ("rmoveto", 2), ("hmoveto", 1),
              ("vmoveto", 1), ("rlineto", 4), ("hlineto", 3), ("vlineto", 3), ("rrcurveto", 6), ("rcurveline", 8), ("rlinecurve", 8),
              ("vvcurveto", 5), ("hhcurveto", 5), ("vhcurveto", 9), ("hvcurveto", 9), ("flex", 13), ("hflex", 7), ("hflex1", 9), ("flex1", 11)]


def _programs():
    p = []
    add = lambda name, cs: p.append((name, cs))   # noqa: E731
    line = enc(7, "hlineto")
    # stack depth: the edge of the LDS window, the limit, one past it
    for n in (WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW + 1, 512, 513, 514):
        add(f"stack_{n}", START + enc(*vals(n, n), "hlineto"))
    add("stack_513_rrcurveto", START + enc(*vals(510, 3), "rrcurveto") + enc(*vals(513, 5), "vlineto"))
    # the window's edge inside one blend (set 0: four deltas per value)
    add("blend_values_below_deltas_above", START + enc(*vals(WINDOW - 8)) + blend(vals(8, 1), 4) + enc("hlineto"))
    add("blend_values_astride", START + enc(*vals(WINDOW - 4)) + blend(vals(8, 2), 4) + enc("hlineto"))
    add("blend_all_above", START + enc(*vals(WINDOW + 12)) + blend(vals(8, 3), 4) + enc("hlineto"))
    add("blend_count_on_the_edge", START + enc(*vals(WINDOW - 10)) + blend(vals(2, 4), 4) + enc("hlineto"))       # n sits in slot 48
    add("blend_count_below_the_edge", START + enc(*vals(WINDOW - 11)) + blend(vals(2, 5), 4) + enc("hlineto"))    # ... in slot 47
    add("blend_below_after_deep", START + enc(*vals(300), "hlineto") + blend(vals(4, 6), 4) + enc("rlineto"))
    add("blend_deep_then_below", START + enc(*vals(20)) + blend(vals(90, 7), 4) + enc("rlineto") + blend(vals(2, 8), 4) + enc("rlineto"))
    add("blend_64_regions_astride", START + select(K64) + enc(*vals(WINDOW - 3)) + blend(vals(6, 9), 64) + enc("hlineto"))
    add("blend_fills_the_stack", START + enc(*vals(2)) + blend(vals(102), 4) + enc("rlineto"))                   # 2 + 510 + the count = 513
    # blend itself
    for s in (K0, K1, K2, K64):
        k = REGIONS_OF[s]
        add(f"blend_k{k}", select(s) + START + blend(vals(2, k), k) + enc("rlineto"))
    add("blend_n0", START + enc(5, 6, 0, "blend", "rlineto"))
    add("blend_n0_alone", START + enc(0, "blend") + line)
    add("blend_exactly_the_stack", START + blend(vals(4), 4) + enc("rlineto"))
    add("blend_one_short", START + line + enc(*vals(19), 4, "blend", "rlineto"))
    add("blend_fraction", START + enc(9, 1, 2, 3, 4, 1.5, "blend", "hlineto"))
    add("blend_fraction_below_1", START + enc(9, 0.5, "blend", 1, "rlineto"))
    add("blend_negative", START + line + enc(9, 1, 2, 3, 4, -1, "blend", "hlineto"))
    add("blend_count_huge", START + line + enc(9, 1, 2, 3, 4, 32767, "blend") + line)
    # (no operand states more than 32767: the count is the sum two blends make, 98301 with set 3's factor 1)
    add("blend_count_past_65535", select(K1) + START + line + enc(32767, 32767, 1, "blend", 32767, 1, "blend", "blend") + line)
    add("blend_empty_stack", START + line + enc("blend") + line)
    add("blend_twice", START + blend([10], 4) + blend([20], 4, 1) + enc("rlineto"))
    add("blend_of_a_blend", START + enc(50) + blend([1], 4) + enc(2, 3, 4, 1, "blend", "hlineto"))    # the first result is a delta of the second
    add("blend_fixed", START + enc(1.5, -0.25, 0.125, 3.0625, 1000.5, 1, "blend", "hlineto"))
    for op, n in _OPERATORS:
        pre = b"" if op in ("rmoveto", "hmoveto", "vmoveto", "hstem", "vstem", "hstemhm", "vstemhm") else START
        mask = b"\x80" if op in ("hintmask", "cntrmask") else b""
        add(f"blend_{op}", pre + blend(vals(n, len(op)), 4, n) + enc(op) + mask + (START if not pre or mask else b"") + line)
    add("blend_callsubr", START + blend([-107], 4) + enc("callsubr") + line)          # default: subroutine 0; other factors: whatever it becomes
    add("blend_callgsubr", START + blend([-107], 4) + enc("callgsubr") + line)
    add("blend_in_subr", START + _call("callsubr", 1) + line)
    add("blend_operands_of_the_caller", START + enc(9, 1, 2, 3, 4) + _call("callsubr", 2) + enc("hlineto"))
    add("blend_depth_10", START + _call(_LVL[1], 11) + line)
    add("depth_11", START + line + _call("callsubr", 21) + line)
    # vsindex
    add("vsindex_k2", select(K2) + START + blend(vals(2), 2) + enc("rlineto"))
    add("vsindex_0", enc(0, "vsindex") + START + blend(vals(2), 4) + enc("rlineto"))
    add("vsindex_after_path", START + line + select(K2) + blend(vals(2), 2) + enc("rlineto"))
    add("vsindex_after_blend", START + blend([5], 4) + enc("hlineto", 1, "vsindex") + line)
    add("vsindex_twice", select(K2) + START + line + select(K1) + line)
    add("vsindex_twice_same", enc(0, "vsindex", 0, "vsindex") + START + line)
    add("vsindex_2_operands", enc(1, 1, "vsindex") + START + line)
    add("vsindex_no_operand", START + line + enc("vsindex") + line)
    add("vsindex_past_count", START + line + select(PAST) + line)
    add("vsindex_unusable", START + line + select(UNUSABLE) + line)
    add("vsindex_too_many_regions", START + line + select(TOO_MANY) + line)
    add("vsindex_negative", START + line + enc(-1, "vsindex") + line)
    add("vsindex_fraction", enc(1.75, "vsindex") + START + blend(vals(2), 2) + enc("rlineto"))
    add("vsindex_in_subr_operand", START + enc(K1) + _call("callgsubr", 21) + enc("vsindex") + blend(vals(2), 1) + enc("rlineto"))   # (global 21 is empty)
    # the ends of a glyph
    add("return_mid_glyph", START + line + enc("return") + line)
    add("endchar_mid_glyph", START + line + enc("endchar") + line)
    add("endchar_last", START + line + enc("endchar"))
    add("return_in_subr", START + line + _call("callsubr", 4) + line)
    add("endchar_in_subr", START + line + _call("callsubr", 5) + line)
    add("mask_past_end", START + line + enc(*range(1, 41), "hintmask", b"\xff"))
    add("mask_past_end_in_subr", START + line + _call("callsubr", 3) + line)
    add("mask_exact", enc(1, 2, 3, 4, "hstemhm", "hintmask", b"\xc0") + START + line)
    add("odd_stems", enc(600, 1, 2, "hstem") + START + line)                       # no width: the odd operand is left over
    add("move_with_width", enc(600, 10, 20, "rmoveto") + line)                     # ... and here it is one operand too many
    add("ends_open", START + enc(5, 5, "rlineto"))
    add("two_contours", START + line + enc(10, "hmoveto") + line)
    add("empty", b"")
    add("escape_unsupported", START + line + enc(1, 2, b"\x0c\x0a") + line)
    for r in (0, 2, 9, 13, 17):
        add(f"reserved_{r}", START + line + enc(1, bytes([r])) + line)
    # the version 1 kit's curve and line cases, without their endchar
    for name, cs in K._curve_cases():
        assert cs.endswith(b"\x0e")
        add("v1_" + name, cs[:-1])
    return p


def shared_face(order=None, name="shared2"):
    loc, glo = _shared_sets()
    progs = _programs()
    if order is not None:
        progs = [progs[i] for i in order]
    return Face(name, [(".notdef", NOTDEF)] + progs, glo, loc)


def set0_unusable_face():
    return Face("set0_unusable", [(".notdef", NOTDEF), ("line", START + enc(7, "hlineto")), ("to_set_1", select(1) + START + enc(7, "hlineto"))],
                sets=[MISSING, [0]])


def no_sets_face():
    return Face("no_sets", [(".notdef", NOTDEF), ("line", START + enc(7, "hlineto")), ("empty", b"")], sets=[])


def sized_face(n, deep_last=0):
    """n glyph ids whose neighbours select different sets and reach different depths of the stack (some past 513);
    deep_last: the last so many glyph ids fill the stack"""
    glyphs = []
    for g in range(n):
        s = (K4, K2, K1, K0)[g % 4]
        k = REGIONS_OF[s]
        depth = (g * 37) % 140 if g % 8 else (514, 47, 48, 49, 513, 300, 520, 96)[(g // 8) % 8]
        if g >= n - deep_last:
            depth = 512 - (n - 1 - g)
        cs = select(s) + enc(g % 50, g % 31, "rmoveto") + blend(vals(2, g), k, g) + enc("rlineto")
        if depth:
            cs += enc(*vals(depth, g), "hlineto")
        glyphs.append((f"g{g}", cs))
    return Face(f"sized2_{n}", glyphs)


def chunk_face(n=16385):
    """three-byte glyphs (one move each), for the boundary between two launches; the glyph ids on either side of it fill the stack"""
    glyphs = [(f"g{g}", enc(g % 200 - 100, (g // 200) % 200 - 100, "rmoveto")) for g in range(n)]
    assert all(len(cs) == 3 for _, cs in glyphs)
    for g in (16383, 16384):
        if g < n:
            glyphs[g] = (f"deep{g}", START + enc(*vals(507, g)) + blend([g % 100], 4, g) + enc("hlineto"))   # 507 + 6: the whole stack
    return Face(f"chunk_{n}", glyphs)


def budget_faces():
    """nested local subroutines of fan-out 4 that end with their data (T(leaf) = 1, T(k) = 4 (2 + T(k - 1))), called so that the
    charstring executes exactly MAX_TOKENS tokens — and one more"""
    t = [1]
    for _ in range(8):
        t.append(4 * (2 + t[-1]))
    subrs = [enc("hstem")] + [_call("callsubr", k - 1) * 4 for k in range(1, 9)]
    left = MAX_TOKENS - 2 - 4                    # "0 hmoveto" in front, "1 hlineto 1 vlineto" behind
    body = b""
    for k in range(8, -1, -1):
        c, left = divmod(left, 2 + t[k])
        body += _call("callsubr", k) * c
    pad = enc("hstem") * left
    at = pad + enc(0, "hmoveto") + body + enc(1, "hlineto", 1, "vlineto")
    small = START + enc(5, "hlineto")
    return [Face("at_budget2", [(".notdef", NOTDEF), ("at", at)], [], subrs),
            Face("over_budget2", [(".notdef", NOTDEF), ("small", small), ("over", enc("hstem") + at)], [], subrs, refusal="budget")]
