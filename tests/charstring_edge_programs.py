"""A kit (no tests): hand-written Type 2 charstring programs at the edges of the interpreter's rules, the `CFF ` tables that
hold them, and a strict sequential interpreter that says what every program delivers.

The interpreter is written from the rules of csrc/host/cff.cpp (CharStringRun) and from Technical Notes #5176 / #5177,
independently of fontTools, which does not model the failure points: an operand cut off by the end of its stream, the 49th
operand, the 11th nested call, a subroutine index outside its set, a mask that runs past the end, a second width, a path
operator in front of the first move, data after endchar.  A program that fails midway keeps the callbacks delivered up to there.
It reads the DESCRIPTION of a face (vgsdf_font_charstrings_desc as a dict of numpy arrays: what FontManager.charstring_font_desc
returns), so it checks the description too.

The `CFF ` tables are written here byte by byte (INDEX offSize chosen by the caller, DICT offsets as five-byte integers, so the
layout needs no second pass) and put into an OpenType shell made with fontTools' FontBuilder.
"""
import io
import struct
from dataclasses import dataclass, field

import numpy as np

MAX_OPERANDS, MAX_DEPTH, MAX_TOKENS = 48, 10, 1 << 20   # charstring_limits.h, VGSDF_CHARSTRING_MAX_TOKENS
M, L, C, Z = 0, 1, 3, 4                                  # command kinds of the packed form

OP = {"hstem": b"\x01", "vstem": b"\x03", "vmoveto": b"\x04", "rlineto": b"\x05", "hlineto": b"\x06", "vlineto": b"\x07",
      "rrcurveto": b"\x08", "callsubr": b"\x0a", "return": b"\x0b", "endchar": b"\x0e", "hstemhm": b"\x12", "hintmask": b"\x13",
      "cntrmask": b"\x14", "rmoveto": b"\x15", "hmoveto": b"\x16", "vstemhm": b"\x17", "rcurveline": b"\x18", "rlinecurve": b"\x19",
      "vvcurveto": b"\x1a", "hhcurveto": b"\x1b", "callgsubr": b"\x1d", "vhcurveto": b"\x1e", "hvcurveto": b"\x1f",
      "hflex": b"\x0c\x22", "flex": b"\x0c\x23", "hflex1": b"\x0c\x24", "flex1": b"\x0c\x25"}


def bias(n):
    return 107 if n < 1240 else (1131 if n < 33900 else 32768)


def num(v):
    """an operand in its shortest form (a float: 16.16 fixed, operator 255)"""
    if isinstance(v, float):
        return b"\xff" + struct.pack(">i", int(round(v * 65536.0)))
    if -107 <= v <= 107:
        return bytes([v + 139])
    if 108 <= v <= 1131:
        return bytes([247 + ((v - 108) >> 8), (v - 108) & 255])
    if -1131 <= v <= -108:
        return bytes([251 + ((-v - 108) >> 8), (-v - 108) & 255])
    return b"\x1c" + struct.pack(">h", v)


def enc(*items):
    """a program: ints / floats are operands, strings operators, bytes go in as they are"""
    out = b""
    for it in items:
        out += it if isinstance(it, bytes) else (OP[it] if isinstance(it, str) else num(it))
    return out


# ---- the interpreter ---------------------------------------------------------------------------------------------------------

@dataclass
class Outcome:
    kinds: list = field(default_factory=list)
    coords: list = field(default_factory=list)   # np.float32
    end: str = ""        # "endchar" | "end" (the stream ran out) | "return" (at the top level) | "fail" | "seac" | "budget"
    tokens: int = 0      # executed tokens, operands and operators alike (the one that passed the budget included)


class _Stop(Exception):
    pass


def interpret(desc, gid, budget=MAX_TOKENS, trace=None):
    """trace: called as trace(op, data, pos, end, stack, depth, st) for every token about to be executed, pos behind its first
    byte (and once more, with op = (12, second byte), for an escaped operator)"""
    data = desc["bytes"].tobytes() if not isinstance(desc["bytes"], (bytes, bytearray)) else desc["bytes"]
    cs_off, gs_off, ls_off, ls_first = desc["cs_off"], desc["gsubr_off"], desc["lsubr_off"], desc["lsubr_first"]
    fd = 0 if desc.get("fd_of") is None else int(desc["fd_of"][gid])
    l0, n_local, n_global = int(ls_first[fd]), int(ls_first[fd + 1]) - int(ls_first[fd]), len(gs_off) - 1
    f32 = np.float32
    out = Outcome()
    stack = []
    st = {"x": f32(0), "y": f32(0), "has_move": False, "first_move": True, "width": False, "endchar": False, "stems": 0}

    def stop(why):
        out.end = why
        raise _Stop()

    def emit(kind, *v):
        out.kinds.append(kind)
        out.coords.extend(v)

    def curve_rel(i):
        x1, y1 = st["x"] + stack[i], st["y"] + stack[i + 1]
        x2, y2 = x1 + stack[i + 2], y1 + stack[i + 3]
        st["x"], st["y"] = x2 + stack[i + 4], y2 + stack[i + 5]
        emit(C, x1, y1, x2, y2, st["x"], st["y"])

    def need(ok):
        if not ok:
            stop("fail")

    def run(pos, end, depth):
        """True: the stream returned (ran out, `return`, or a successful endchar)"""
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
                need(len(stack) < MAX_OPERANDS)
                stack.append(v)
                continue
            sp = len(stack)
            if op in (1, 3, 18, 23):
                n = sp
                if (n & 1) and not st["width"]:
                    st["width"] = True
                    n -= 1
                st["stems"] += n >> 1
                stack.clear()
            elif op in (19, 20):
                n = sp
                stack.clear()
                if n & 1:
                    n -= 1
                    st["width"] = True
                st["stems"] += n >> 1
                need((st["stems"] + 7) >> 3 <= end - pos)
                pos += (st["stems"] + 7) >> 3
            elif op in (21, 22, 4):
                hx, hy = op != 4, op != 22
                want = hx + hy
                skip = 0
                if sp == want + 1 and not st["width"]:
                    skip = 1
                    st["width"] = True
                need(sp == skip + want)
                if st["first_move"]:
                    st["first_move"] = False
                else:
                    emit(Z)
                st["has_move"] = True
                i = skip
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
                need(float(fidx) == int(fidx))
                idx = int(fidx) + bias(n)
                need(0 <= idx < n)
                off = gs_off if op == 29 else ls_off[l0:]
                run(int(off[idx]), int(off[idx + 1]), depth + 1)
                if st["endchar"]:
                    need(pos == end)      # data after endchar
                    return True
            elif op == 11:
                if depth == 0:
                    out.end = "return"
                return True
            elif op == 14:
                if sp == 4 or (not st["width"] and sp == 5):
                    stop("seac")
                if sp == 1 and not st["width"]:
                    st["width"] = True
                stack.clear()
                if not st["first_move"]:
                    st["first_move"] = True
                    emit(Z)
                need(pos == end)          # data after endchar
                st["endchar"] = True
                return True
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
                stop("fail")              # 0, 2, 9, 13, 15, 16, 17
        return True

    try:
        run(int(cs_off[gid]), int(cs_off[gid + 1]), 0)
        if not out.end:
            out.end = "endchar" if st["endchar"] else "end"
    except _Stop:
        pass
    return out


def expected_commands(desc, budget=MAX_TOKENS):
    """the face's command description (the dict FontManager.command_font_desc returns) by the interpreter, and every glyph id's
    end state"""
    n = len(desc["cs_off"]) - 1
    cmd_off, dat_off, kinds, coords, ends = [0], [0], [], [], []
    for g in range(n):
        o = interpret(desc, g, budget)
        kinds += o.kinds
        coords += o.coords
        cmd_off.append(len(kinds))
        dat_off.append(len(coords))
        ends.append(o.end)
    return {"cmd_off": np.array(cmd_off, np.uint32), "dat_off": np.array(dat_off, np.uint32), "kinds": np.array(kinds, np.uint8),
            "coords": np.array(coords, np.float32)}, ends


# ---- `CFF ` tables by hand ---------------------------------------------------------------------------------------------------

def _index(items, off_size=None):
    if not items:
        return b"\x00\x00"
    offs = [1]
    for it in items:
        offs.append(offs[-1] + len(it))
    need = 1 if offs[-1] < 1 << 8 else 2 if offs[-1] < 1 << 16 else 3 if offs[-1] < 1 << 24 else 4
    off_size = off_size or need
    assert off_size >= need, "INDEX data too long for the offSize asked for"
    return struct.pack(">HB", len(items), off_size) + b"".join(o.to_bytes(off_size, "big") for o in offs) + b"".join(items)


def _int5(v):
    return b"\x1d" + struct.pack(">i", v)


def _private(lsubrs, off_size):
    """a Private DICT and, right behind it, its local subroutines"""
    if not lsubrs:
        return bytes([139, 20]), b""       # defaultWidthX 0
    return _int5(6) + b"\x13", _index(lsubrs, off_size)


def cff_table(charstrings, gsubrs=(), lsubr_sets=((),), fd_of=None, off_size=None):
    """charstrings: bytes per glyph id.  fd_of None: a name-keyed font with the one local set; otherwise CID-keyed with one Font
    DICT per set and an FDSelect of format 0 (fd_of: one index per glyph id).  off_size: forced on every INDEX (None: the smallest)"""
    n = len(charstrings)
    cid = fd_of is not None
    strings = [b"Adobe", b"Identity"] if cid else [b"g%d" % i for i in range(1, n)]
    head = b"\x01\x00\x04\x04" + _index([b"Synth"], off_size)
    top_len = 6 + 6 + (13 + 7 + 7 if cid else 11)
    tail = _index(strings, off_size) + _index(list(gsubrs), off_size)
    at = len(head) + len(_index([b"\0" * top_len], off_size)) + len(tail)
    charset_at = at
    body = b"\x00" + b"".join(struct.pack(">H", i if cid else 390 + i) for i in range(1, n))   # charset format 0
    fdselect_at = at + len(body)
    if cid:
        body += b"\x00" + bytes(fd_of)
    cs_at = at + len(body)
    body += _index(list(charstrings), off_size)
    top = _int5(charset_at) + b"\x0f" + _int5(cs_at) + b"\x11"
    if cid:
        privs = [_private(list(s), off_size) for s in lsubr_sets]
        fdarray_at = at + len(body)
        blob_at = fdarray_at + len(_index([b"\0" * 11] * len(privs), off_size))
        fds, blob = [], b""
        for d, subrs in privs:
            fds.append(_int5(len(d)) + _int5(blob_at + len(blob)) + b"\x12")
            blob += d + subrs
        body += _index(fds, off_size) + blob
        top = _int5(391) + _int5(392) + bytes([139]) + b"\x0c\x1e" + top + _int5(fdarray_at) + b"\x0c\x24" + _int5(fdselect_at) + b"\x0c\x25"
    else:
        d, subrs = _private(list(lsubr_sets[0]), off_size)
        top += _int5(len(d)) + _int5(at + len(body)) + b"\x12"
        body += d + subrs
    assert len(top) == top_len
    return head + _index([top], off_size) + tail + body


_SHELLS = {}


def _shell(n_glyphs):
    """an OpenType font of n_glyphs glyph ids around a `CFF ` table (built once per count): glyph id i >= 1 at code point
    0x100 + i, advance 600"""
    if n_glyphs not in _SHELLS:
        from fontTools.fontBuilder import FontBuilder
        from fontTools.misc.psCharStrings import T2CharString
        names = [".notdef"] + [f"g{i}" for i in range(1, n_glyphs)]
        fb = FontBuilder(1000, isTTF=False)
        fb.setupGlyphOrder(names)
        fb.setupCharacterMap({0x100 + i: names[i] for i in range(1, min(n_glyphs, 0xFE00))})
        fb.setupCFF("Synth", {}, {g: T2CharString(program=["endchar"]) for g in names}, {})
        fb.setupHorizontalMetrics({g: (600, 0) for g in names})
        fb.setupHorizontalHeader(ascent=935, descent=-265)
        fb.setupNameTable({"familyName": "Synth Edge", "styleName": "Regular"})
        fb.setupOS2()
        fb.setupPost()
        buf = io.BytesIO()
        fb.save(buf)
        _SHELLS[n_glyphs] = buf.getvalue()
    return _SHELLS[n_glyphs]


def otf(cff, n_glyphs):
    """the table in its OpenType shell"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    font = TTFont(io.BytesIO(_shell(n_glyphs)), recalcBBoxes=False, recalcTimestamp=False)   # (no table looks into `CFF ` on saving)
    raw = DefaultTable("CFF ")
    raw.data = cff
    font["CFF "] = raw
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


def glyph_commands(d, g):
    """glyph id g of a command description (cmd_off / dat_off / kinds / coords) as bytes: (kinds, coordinates bit for bit)"""
    return (d["kinds"][d["cmd_off"][g]:d["cmd_off"][g + 1]].tobytes(), d["coords"][d["dat_off"][g]:d["dat_off"][g + 1]].tobytes())


@dataclass
class Face:
    name: str
    glyphs: list                  # (name, charstring bytes); glyph id 0 is .notdef
    gsubrs: list = field(default_factory=list)
    lsubr_sets: list = field(default_factory=lambda: [[]])
    fd_of: list = None            # CID-keyed: one Font DICT index per glyph id
    refusal: str = ""             # "seac" / "budget": what the device refuses the face for

    def cff(self, off_size=None):
        return cff_table([g for _, g in self.glyphs], self.gsubrs, self.lsubr_sets, self.fd_of, off_size)

    def font(self, off_size=None):
        return otf(self.cff(off_size), len(self.glyphs))

    def desc(self):
        """the description as the host would state it (bodies in INDEX order: charstrings, global, local sets)"""
        blob, offs = b"", {}
        for key, items in (("cs_off", [g for _, g in self.glyphs]), ("gsubr_off", self.gsubrs)):
            o = [len(blob)]
            for it in items:
                blob += it
                o.append(len(blob))
            offs[key] = np.array(o, np.uint32)
        first, lo = [0], [len(blob)]
        for s in self.lsubr_sets:
            for it in s:
                blob += it
                lo.append(len(blob))
            first.append(len(lo) - 1)
        blob += b"\0" * (-len(blob) % 4)
        return {"bytes": np.frombuffer(blob, np.uint8).copy(), **offs, "lsubr_first": np.array(first, np.uint32),
                "lsubr_off": np.array(lo, np.uint32),
                "fd_of": None if len(self.lsubr_sets) == 1 else np.array(self.fd_of, np.uint8)}


# ---- the programs ------------------------------------------------------------------------------------------------------------

NOTDEF = enc(0, "hmoveto", "endchar")
RET = enc("return")

# the subroutines most programs share (fewer than 1240 in either set: bias 107).  Levels 1 .. 10 of a call chain alternate
# between the sets: level j is subroutine 10 + j of the local set for odd j, of the global set for even j
_LVL = {j: ("callsubr" if j % 2 else "callgsubr") for j in range(1, 12)}


def _call(kind, index):
    return enc(index - 107, kind)


def _shared_sets():
    loc, glo = [RET] * 22, [RET] * 22
    loc[0] = enc(10, 20, "rlineto", "return")
    loc[1] = enc("endchar")                                  # endchar inside a subroutine
    loc[2] = enc(5, 5, "rlineto")                            # ends with its data, no return
    loc[3] = enc("endchar", 1)                               # data after endchar, inside the subroutine
    loc[4] = enc(7, "return")                                # leaves an operand for the caller
    glo[0] = enc(-5, 40, "rlineto", "return")
    glo[1] = enc(1, 2, 3, 4, 5, 6, "rrcurveto", -107, "callgsubr", "return")
    glo[2] = enc(9, 9, "rlineto", "endchar")
    glo[3] = _call("callsubr", 1) + enc(3, 3, "rlineto")     # calls the endchar subroutine, data behind the call
    for j in range(1, 11):
        body = enc(1, 2, "rlineto", "return") if j == 10 else _call(_LVL[j + 1], 10 + j + 1) + enc("return")
        (loc if j % 2 else glo)[10 + j] = body
    loc[21] = _call(_LVL[1], 11) + enc("return")             # one level in front of the chain: its level 10 would be the 11th call
    return loc, glo


START = enc(100, 100, "rmoveto")


def _curve_cases():
    out = []
    six = [1, 2, 3, 4, 5, 6]
    def many(k):
        return [((i * 7) % 23) - 9 for i in range(k)]
    for op, counts in (("rrcurveto", (6, 12, 7, 5)), ("rcurveline", (8, 14, 6, 9, 2)), ("rlinecurve", (8, 10, 12, 9, 6)),
                       ("vvcurveto", (4, 5, 8, 9, 6, 7, 3)), ("hhcurveto", (4, 5, 8, 9, 6, 7, 3)),
                       ("hvcurveto", (4, 5, 8, 9, 12, 13, 3, 6, 7, 10, 11)), ("vhcurveto", (4, 5, 8, 9, 12, 13, 3, 6, 7, 10, 11)),
                       ("rlineto", (2, 4, 3)), ("hlineto", (1, 2, 5)), ("vlineto", (1, 2, 5))):
        for k in counts:
            out.append((f"{op}_{k}", START + enc(*many(k), op, 50, "hlineto", "endchar")))
    del six
    return out


def _programs():
    p = []
    add = lambda name, cs: p.append((name, cs))   # noqa: E731
    # number forms at their edges: 246 | 247, 250 | 251, 254 | 255, and 28
    add("numbers", enc(bytes([246]), bytes([247, 0]), "rmoveto", bytes([250, 255]), bytes([251, 0]), "rlineto", bytes([254, 255]), bytes([32]),
                       "rlineto", b"\xff\x7f\xff\xff\xff", b"\xff\x80\x00\x00\x00", "rlineto", b"\xff\x00\x00\x80\x00", b"\xff\xff\xff\xff\xff",
                       "rlineto", b"\x1c\x7f\xff", b"\x1c\x80\x00", "rlineto", 1.5, -2.25, 0.125, 3.0, 1000.0625, -0.5, "rrcurveto", "endchar"))
    for name, cut in (("cut_247", b"\xf7"), ("cut_251", b"\xfb"), ("cut_28_0", b"\x1c"), ("cut_28_1", b"\x1c\x12"),
                      ("cut_255_0", b"\xff"), ("cut_255_3", b"\xff\x00\x00\x01")):
        add(name, START + enc(5, "hlineto", 7) + cut)
    add("stack_48", START + enc(*range(48), "rlineto", "endchar"))
    add("stack_49", START + enc(*range(49), "rlineto", "endchar"))
    add("depth_10", START + _call(_LVL[1], 11) + enc(5, "hlineto", "endchar"))
    add("depth_11", START + _call("callsubr", 21) + enc(5, "hlineto", "endchar"))
    add("subr_below_0", START + enc(-108, "callsubr", 5, "hlineto", "endchar"))
    add("subr_past_count", START + enc(22 - 107, "callsubr", 5, "hlineto", "endchar"))
    add("gsubr_past_count", START + enc(22 - 107, "callgsubr", 5, "hlineto", "endchar"))
    add("subr_fraction", START + enc(-106.5, "callsubr", 5, "hlineto", "endchar"))
    add("subr_no_operand", START + enc("callsubr", 5, "hlineto", "endchar"))
    add("subr_operand_back", START + _call("callsubr", 4) + enc("hlineto", "endchar"))
    add("subr_no_return", START + _call("callsubr", 2) + enc(5, "hlineto", "endchar"))
    add("subrs_mixed", START + _call("callsubr", 0) + _call("callgsubr", 0) + _call("callgsubr", 1) + enc("endchar"))
    # hint masks
    add("mask_0_stems", enc("hintmask") + START + enc(5, "hlineto", "endchar"))
    add("mask_8_stems", enc(*range(16), "hstemhm", "hintmask", b"\xaa") + START + enc(5, "hlineto", "cntrmask", b"\x55", 6, "vlineto", "endchar"))
    add("mask_9_stems", enc(*range(16), "hstemhm", 1, 2, "vstemhm", "hintmask", b"\xaa\x80") + START + enc(5, "hlineto", "endchar"))
    add("mask_9_stems_short", enc(*range(16), "hstemhm", 1, 2, "vstemhm", "hintmask", b"\xaa") + START + enc(5, "hlineto", "endchar"))
    add("mask_past_end", START + enc(5, "hlineto", 1, 2, "hstemhm", "hintmask"))
    add("mask_implied_vstem", enc(1, 2, "hstemhm", 3, 4, "hintmask", b"\xc0") + START + enc(5, "hlineto", "endchar"))
    add("mask_implied_vstem_width", enc(600, 1, 2, "hstemhm", 3, 4, 5, 6, "cntrmask", b"\xe0") + START + enc(5, "hlineto", "endchar"))
    # the width operand: every operator that can take it, and a second one
    for op in ("hstem", "vstem", "hstemhm", "vstemhm"):
        add(f"width_{op}", enc(600, 1, 2, op) + START + enc(5, "hlineto", "endchar"))
    add("width_hintmask", enc(600, 1, 2, "hintmask", b"\x80") + START + enc(5, "hlineto", "endchar"))
    add("width_cntrmask", enc(600, 1, 2, "cntrmask", b"\x80") + START + enc(5, "hlineto", "endchar"))
    add("width_rmoveto", enc(600, 10, 20, "rmoveto", 5, "hlineto", "endchar"))
    add("width_hmoveto", enc(600, 10, "hmoveto", 5, "hlineto", "endchar"))
    add("width_vmoveto", enc(600, 10, "vmoveto", 5, "hlineto", "endchar"))
    add("width_endchar", enc(600, "endchar"))
    add("width_twice_hmoveto", enc(600, 1, 2, "hstem", 9, 5, "hmoveto", 5, "hlineto", "endchar"))
    add("width_twice_rmoveto", enc(600, 10, 20, "rmoveto", 5, "hlineto", 600, 1, 2, "rmoveto", 5, "hlineto", "endchar"))
    add("width_twice_endchar", enc(600, 10, "hmoveto", 5, "hlineto", 600, "endchar"))
    add("move_short", enc("rmoveto", 5, "hlineto", "endchar"))
    add("moves_close", START + enc(5, "hlineto", 10, "hmoveto", 5, "vlineto", 10, "vmoveto", 1, 1, "rlineto", 3, 4, "rmoveto", "endchar"))
    # path operators in front of the first move
    for op, k in (("rlineto", 2), ("hlineto", 1), ("vlineto", 1), ("rrcurveto", 6), ("rcurveline", 8), ("rlinecurve", 8), ("vvcurveto", 4),
                  ("hhcurveto", 4), ("hvcurveto", 4), ("vhcurveto", 4), ("flex", 13), ("hflex", 7), ("hflex1", 9), ("flex1", 11)):
        add(f"no_move_{op}", enc(*range(1, k + 1), op) + START + enc(5, "hlineto", "endchar"))
    p.extend(_curve_cases())
    # flex
    add("flex", START + enc(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 50, "flex", 5, "hlineto", "endchar"))
    add("flex_12", START + enc(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, "flex", 5, "hlineto", "endchar"))
    add("hflex", START + enc(10, 20, 30, 40, 50, 60, 70, "hflex", 5, "hlineto", "endchar"))
    add("hflex_8", START + enc(10, 20, 30, 40, 50, 60, 70, 80, "hflex", 5, "hlineto", "endchar"))
    add("hflex1", START + enc(10, 20, 30, 40, 50, 60, 70, 80, 90, "hflex1", 5, "hlineto", "endchar"))
    add("hflex1_8", START + enc(10, 20, 30, 40, 50, 60, 70, 80, "hflex1", 5, "hlineto", "endchar"))
    add("flex1_dx", START + enc(10, 1, 10, 1, 10, 1, 10, 1, 10, 1, 7, "flex1", 5, "hlineto", "endchar"))
    add("flex1_dy", START + enc(1, 10, 1, 10, 1, 10, 1, 10, 1, 10, 7, "flex1", 5, "hlineto", "endchar"))
    add("flex1_equal", START + enc(1, 2, 3, 4, 5, 6, 6, 5, 4, 3, 7, "flex1", 5, "hlineto", "endchar"))
    add("flex1_equal_signs", START + enc(1, 2, 3, 4, 5, 6, 6, 5, 4, -27, 7, "flex1", 5, "hlineto", "endchar"))
    add("flex1_10", START + enc(1, 2, 3, 4, 5, 6, 6, 5, 4, 3, "flex1", 5, "hlineto", "endchar"))
    # escape and reserved operators, midway through a path
    add("escape_unsupported", START + enc(5, "hlineto", 1, 2, b"\x0c\x0a", 6, "vlineto", "endchar"))
    add("escape_cut", START + enc(5, "hlineto", b"\x0c"))
    for r in (0, 2, 9, 13, 15, 16, 17):
        add(f"reserved_{r}", START + enc(5, "hlineto", 1, bytes([r]), 6, "vlineto", "endchar"))
    # end of stream
    add("endchar_in_subr", START + enc(5, "hlineto") + _call("callsubr", 1))
    add("endchar_in_subr_data_behind_call", START + enc(5, "hlineto") + _call("callsubr", 1) + enc(6, "vlineto"))
    add("endchar_in_subr_with_data", START + enc(5, "hlineto") + _call("callsubr", 3))
    add("endchar_two_levels_down", START + enc(5, "hlineto") + _call("callgsubr", 3))
    add("endchar_in_gsubr", START + _call("callgsubr", 2))
    add("data_after_endchar", START + enc(5, "hlineto", "endchar", 6, "vlineto"))
    add("no_endchar", START + enc(5, "hlineto"))
    add("return_at_top", START + enc(5, "hlineto", "return", 6, "vlineto", "endchar"))
    add("empty", b"")
    add("only_endchar", enc("endchar"))
    return p


def shared_face(order=None, name="shared"):
    """every program that lives with the shared subroutines, one glyph id each behind .notdef; order: a permutation of them"""
    loc, glo = _shared_sets()
    progs = _programs()
    if order is not None:
        progs = [progs[i] for i in order]
    return Face(name, [(".notdef", NOTDEF)] + progs, glo, [loc])


def single_faces():
    """the programs as one face each (glyph id 1 behind .notdef)"""
    loc, glo = _shared_sets()
    return [Face(n, [(".notdef", NOTDEF), (n, cs)], glo, [loc]) for n, cs in _programs()]


def _bias_glyphs(n, kind):
    b = bias(n)
    # (an index whose operand no charstring can state is left out: one below 0 at bias 32768, one past 33899 at bias 1131)
    cases = [("first", 0), ("last", n - 1), ("past_count", n), ("below_0", -1), ("as_bias_107", b - 107), ("as_bias_1131", b - 1131)]
    return [(".notdef", NOTDEF)] + [(name, START + enc(idx - b, kind, 5, "hlineto", "endchar")) for name, idx in cases
                                    if -32768 <= idx - b <= 32767]


def bias_faces():
    """subroutine counts on both sides of the two bias steps; the bodies are one-byte returns"""
    out = []
    for n in (1239, 1240):
        out.append(Face(f"local_{n}", _bias_glyphs(n, "callsubr"), [], [[RET] * n]))
    for n in (33899, 33900):
        out.append(Face(f"global_{n}", _bias_glyphs(n, "callgsubr"), [RET] * n, [[]]))
    return out


def cid_face():
    """CID-keyed: three Font DICTs whose local sets (1239, 1240 and 3 subroutines) lie on both sides of a bias step; the same
    operands name other subroutines, or none, depending on the glyph's Font DICT"""
    sets = [[enc(1, 1, "rlineto", "return")] * 1239, [enc(2, 2, "rlineto", "return")] * 1240, [enc(3, 3, "rlineto", "return")] * 3]
    glyphs, fd_of = [(".notdef", NOTDEF)], [0]
    for operand in (-107, -105, -104, 0, 108, 1131, 1132, -1131, -1132, 1239 - 1131 - 1, 1239 - 107):
        for fd in (0, 1, 2):
            glyphs.append((f"op{operand}_fd{fd}", START + enc(operand, "callsubr", 5, "hlineto", "endchar")))
            fd_of.append(fd)
    return Face("cid", glyphs, [enc(4, 4, "rlineto", "return")], sets, fd_of)


def seac_faces():
    std = [(".notdef", NOTDEF), ("A", START + enc(5, "hlineto", "endchar"))]
    return [Face("seac_width", std + [("Aacute", enc(640, 150, 700, 65, 194, "endchar"))], refusal="seac"),
            Face("seac_no_width", std + [("Aacute", enc(150, 700, 65, 194, "endchar"))], refusal="seac"),
            Face("seac_behind_a_path", std + [("Aacute", enc(600, 1, "hmoveto", 150, 700, 65, 194, "endchar"))], refusal="seac")]


def budget_faces():
    """nested local subroutines of fan-out 4 (T(leaf) = 1, T(k) = 9 + 4 T(k + 1): 13, 61, ... 262141), called so that the
    charstring executes exactly MAX_TOKENS tokens — and one more (a leading hstem on an empty stack)"""
    t = [1]
    for _ in range(8):
        t.append(9 + 4 * t[-1])           # t[k]: tokens of the subroutine k levels above the leaf
    # local subroutine k = the one k levels above the leaf
    subrs = [RET] + [_call("callsubr", k - 1) * 4 + RET for k in range(1, 9)]
    # 3 x (2 + T8) + 4 x (2 + T7) = 786429 + 262140; the remaining 7 tokens: three drawing pairs and endchar
    assert 3 * (2 + t[8]) + 4 * (2 + t[7]) + 7 == MAX_TOKENS
    body = _call("callsubr", 8) * 3 + _call("callsubr", 7) * 4
    at = enc(0, "hmoveto") + body + enc(1, "hlineto", 1, "vlineto", "endchar")
    return [Face("at_budget", [(".notdef", NOTDEF), ("at", at)], [], [subrs]),
            Face("over_budget", [(".notdef", NOTDEF), ("small", START + enc(5, "hlineto", "endchar")), ("over", enc("hstem") + at)],
                 [], [subrs], refusal="budget")]


def sized_face(n, empty=()):
    """n glyph ids of small distinct programs; the glyph ids of `empty` have an empty charstring"""
    glyphs = []
    for g in range(n):
        cs = b"" if g in empty else enc(g % 50, g % 31, "rmoveto", *[(g * (i + 3)) % 17 - 8 for i in range(2 * (1 + g % 5))], "rlineto", "endchar")
        glyphs.append((f"g{g}", cs))
    return Face(f"sized_{n}", glyphs)


def long_face():
    """one charstring of a few thousand tokens (glyph id 17) among 63 of one token"""
    long = START
    for i in range(400):
        long += enc((i % 13) - 6, (i % 7) - 3, (i % 5) - 2, (i % 11) - 5, (i % 3) - 1, (i % 17) - 8, "rrcurveto", i % 9 - 4, "hlineto")
    long += enc("endchar")
    return Face("long", [(f"g{g}", long if g == 17 else enc("endchar")) for g in range(64)])
