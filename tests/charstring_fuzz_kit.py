"""A kit (no tests): seeded random Type 2 and CFF2 charstring faces on top of the hand-written kits
(tests/charstring_edge_programs.py, tests/charstring2_edge_programs.py), whose table writers and strict interpreters it uses.

face(seed, cff2, n) draws every glyph of a face from a grammar: stems in the four spellings and masks (the implicit vstem, stem
counts on both sides of 8, 16 and 96), the width operand under every operator that may carry it, every path operator in every
argument-count form, the five operand spellings, `blend` over 0, 1, 2, 4 and 64 regions with operands on both sides of the LDS
window's edge, operand stacks up to the limits, and then moves random spans of the token list into local and global
subroutines, nested up to ten deep, wherever the span happens to begin and end: operands are left on the stack across calls and
returns.  A bounded share of the programs fails by the interpreter's rules; what such a glyph delivers is what the interpreter
says.  Every glyph is run by the kit's interpreter when it is made and kept only if that run ends within MAX_RUN_TOKENS.

Three more readings of a face for the tests: features() (what a run reached, derived from the interpreter's trace and not from
the generator's intent: FEATURES lists what a corpus must reach), tracked_run() (the interpreter over numbers that count their own
f32 roundings: the bound for a reader that works in f64) and MUTANTS (the interpreters with one rule broken each).
"""
import inspect
import math
import operator
import random
import struct

import numpy as np

import charstring_edge_programs as K
import charstring2_edge_programs as K2

MAX_RUN_TOKENS = 4096
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)          # the corpus of the tests: one face of each version per seed
N_GLYPHS = 192
_OPB = dict(K.OP, **K2._OP2)
_STEMS = ("hstem", "vstem", "hstemhm", "vstemhm")
_MOVES = {"rmoveto": 2, "hmoveto": 1, "vmoveto": 1}
_STEM_TOTALS = (1, 7, 8, 9, 15, 16, 17, 95, 96, 97)
_SET_SIZES = (4, 30, 108, 1239, 1240, 1241)


# ---- the generator -----------------------------------------------------------------------------------------------------------

def _spell(rng, v, fixed=True):
    """operand v in one of the spellings that can hold it: the shortest, or a longer one (fixed: 16.16 among them)"""
    if isinstance(v, float):
        if v != int(v) or not -32768 <= v <= 32767:
            return K.num(v)
        v = int(v)
    r = rng.random()
    if r < 0.12 and -32768 <= v <= 32767:
        return b"\x1c" + struct.pack(">h", v)
    if fixed and r < 0.22 and -32768 <= v <= 32767:
        return K.num(float(v))
    return K.num(v)


class _Builder:
    def __init__(self, rng, cff2, n_local, n_global):
        self.rng, self.cff2 = rng, cff2
        self.n = {"l": n_local, "g": n_global}
        self.subrs = {"l": {}, "g": {}}
        self.free = {k: self._slots(n) for k, n in self.n.items()}
        self.known = {}
        self.mode, self.k, self.width = "exact", 4, False

    def _slots(self, n):
        """the indices that get a body, in the order they are handed out: the biased operands 0 and -107, the last, the first"""
        b = K.bias(n)
        first = [i for i in (b, b - 107, n - 1, 0, 1) if 0 <= i < n]
        rest = [i for i in range(n) if i not in first]
        self.rng.shuffle(rest)
        out = []
        for i in first + rest[:400]:
            if i not in out:
                out.append(i)
        return out

    # operands
    def val(self):
        rng, r = self.rng, self.rng.random()
        if self.mode == "inexact" and r < 0.5:
            return rng.randint(-2000000, 2000000) / 65536.0
        if r < 0.72:
            return rng.randint(-40, 40)
        if r < 0.88:
            return rng.randint(-300, 300)
        if r < 0.94:
            return rng.randint(-1200, 1200)
        return rng.randint(-320, 320) / 8.0

    def num(self, v=None):
        return _spell(self.rng, self.val() if v is None else v)

    def args(self, m, depth=0, plain_first=0, p_blend=None):
        """tokens that leave m operands on a stack that holds `depth` already; CFF2: some of them as the results of blends"""
        if not self.cff2:
            return [self.num() for _ in range(m)]
        rng, out, done, k = self.rng, [], 0, self.k
        p = (0.25 if m < 30 else 0.5) if p_blend is None else p_blend
        while done < m:
            room = (K2.MAX_OPERANDS2 - (depth + done) - 1) // (k + 1)
            if done >= plain_first and room >= 1 and rng.random() < p:
                n = min(m - done, room, rng.choice((1, 1, 2, 3, 4, rng.randint(1, 12))))
                out += [self.num() for _ in range(n)] + [self.num(rng.randint(-30, 30) if self.mode == "exact" else None) for _ in range(n * k)]
                out += [self.index(n), _OPB["blend"]]
            else:
                n = 1
                out.append(self.num())
            done += n
        return out

    def index(self, v):
        """a subroutine index, a set index or a blend count: never in 16.16 form, which fontTools cannot index with"""
        return _spell(self.rng, v, fixed=False)

    def lead(self):
        if self.width:
            self.width = False
            return [self.num(self.rng.randint(200, 900))]
        return []

    def mask(self, stems, short=0):
        n = max(0, ((stems + 7) >> 3) - short)
        return _OPB[self.rng.choice(("hintmask", "cntrmask"))] + bytes(self.rng.randrange(256) for _ in range(n))

    def path_form(self):
        """(operator, operand count) over every legal form"""
        rng = self.rng
        op = rng.choice(("rlineto", "hlineto", "vlineto", "rrcurveto", "rcurveline", "rlinecurve", "vvcurveto", "hhcurveto", "hvcurveto",
                         "vhcurveto", "hvcurveto", "vhcurveto", "flex", "hflex", "hflex1", "flex1"))
        g = rng.choice((1, 1, 2, 3, rng.randint(1, 5)))
        if op == "rlineto":
            return op, 2 * g
        if op in ("hlineto", "vlineto"):
            return op, rng.randint(1, 8)
        if op == "rrcurveto":
            return op, 6 * min(g, 3)
        if op == "rcurveline":
            return op, 6 * min(g, 3) + 2
        if op == "rlinecurve":
            return op, 2 * g + 6
        if op in ("vvcurveto", "hhcurveto", "hvcurveto", "vhcurveto"):
            return op, 4 * g + rng.randint(0, 1)
        return op, {"flex": 13, "hflex": 7, "hflex1": 9, "flex1": 11}[op]

    def deep_form(self):
        """an operator whose operands fill the stack: to the limit of 48, or (CFF2) over the window's edge and to 513"""
        rng = self.rng
        if not self.cff2:
            return rng.choice((("rlineto", 48), ("hlineto", 48), ("rrcurveto", 48), ("vlineto", 47), ("hvcurveto", 48), ("rlinecurve", 48)))
        n = rng.choice((rng.randint(40, 60), rng.randint(40, 60), rng.randint(61, 140), rng.randint(500, 513), 513))
        return rng.choice((("hlineto", n), ("vlineto", n), ("rlineto", n & ~1), ("rrcurveto", n - n % 6), ("hvcurveto", (n & ~3) + (n & 1))))

    # programs
    def hints(self, t):
        rng, r, stems = self.rng, self.rng.random(), 0
        if r < 0.45:
            total = rng.choice(_STEM_TOTALS) if rng.random() < 0.4 else rng.randint(1, 20)
            implicit = rng.random() < 0.4
            mask = implicit or rng.random() < 0.5
            left = total
            while left > 0:
                k = min(left, rng.randint(1, 23))
                t += self.lead() + self.args(2 * k, p_blend=0.05)
                left -= k
                if not (implicit and left == 0):
                    t.append(_OPB[rng.choice(_STEMS)])
            stems = total
            if mask:
                t.append(self.mask(stems))
        elif r < 0.53:
            t += self.lead() + [self.mask(0)]
        return stems

    def contours(self, t, stems, n_contours, ops_per=(1, 5), deep=0.04):
        rng = self.rng
        for _ in range(n_contours):
            mv = rng.choice(tuple(_MOVES))
            t += self.lead() + self.args(_MOVES[mv]) + [_OPB[mv]]
            for _ in range(rng.randint(*ops_per)):
                if rng.random() < deep:
                    op, n = self.deep_form()
                    t += self.args(n, plain_first=rng.randint(30, 50), p_blend=0.5) + [_OPB[op]]
                    self.no_calls = self.no_calls or n >= (48 if not self.cff2 else 512)
                else:
                    op, n = self.path_form()
                    if op == "flex1" and self.mode == "exact" and rng.random() < 0.4:     # |dx| = |dy|: the tie of its rule (on exact values only:
                        # the reader decides it on f32 positions, so under rounded ones a tie can fall on either side)
                        d = [rng.randint(-30, 30) for _ in range(10)]
                        d[8] += rng.choice((1, -1)) * sum(d[1::2]) - sum(d[0::2])
                        t += [self.num(v) for v in d] + [self.num(), _OPB[op]]
                    else:
                        t += self.args(n) + [_OPB[op]]
                if rng.random() < 0.08:
                    t.append(self.mask(stems))

    def normal(self, long=False):
        rng, t = self.rng, []
        if self.cff2 and self.k != 4 or self.cff2 and rng.random() < 0.1:
            t += [self.index(self.set_index), _OPB["vsindex"]]
        if not self.cff2 and rng.random() < 0.03:
            return self.lead() + [_OPB["endchar"]]
        stems = self.hints(t)
        self.contours(t, stems, rng.randint(12, 20) if long else rng.randint(1, 4), (4, 8) if long else (1, 5), 0.0 if long else 0.05)
        if self.cff2:
            if rng.random() < 0.08:                                  # a mask past the end ends the stream
                more = rng.randint(1, 12)
                t += self.args(2 * more, p_blend=0.0) + [self.mask(stems + more, short=1)[:-1] if rng.random() < 0.3 else self.mask(stems + more, short=1)]
            return t
        r = rng.random()
        if r < 0.86:
            t += self.lead() + [_OPB["endchar"]]
        elif r < 0.90:
            t.append(_OPB["return"])
        return t

    def failing(self):
        """a program that runs into one of the interpreter's failure points, behind and in front of ordinary contours"""
        rng, t = self.rng, []
        kinds = ["underflow", "no_move", "truncated", "outside", "mask", "overflow", "depth"]
        kind = rng.choice(kinds + (["ends"] if self.cff2 else ["after_endchar", "second_width"]))
        self.width = False
        stems = 0
        if kind == "second_width":                                   # a width, and later a move with one operand too many
            t += [self.num(rng.randint(200, 900))] + self.args(1) + [_OPB[rng.choice(("hmoveto", "vmoveto"))]] + self.args(2) + [_OPB["rlineto"]]
        if kind == "no_move":
            op, n = self.path_form()
            t += self.args(n) + [_OPB[op]]
        if kind != "no_move" or rng.random() < 0.5:
            self.contours(t, stems, rng.randint(1, 2), (1, 3), 0.0)
        cut = None
        if kind == "underflow":
            op, n = rng.choice((("rrcurveto", 5), ("flex", 12), ("hflex", 6), ("rcurveline", 6), ("rmoveto", 1 if self.cff2 else 0), ("callsubr", 0),
                                ("hvcurveto", 3), ("vvcurveto", 6), ("rlineto", 3), ("hlineto", 0), ("blend" if self.cff2 else "flex1", 0)))
            t += self.args(n, p_blend=0.0) + [_OPB[op]]
        elif kind == "truncated":
            cut = rng.choice((b"\xf7", b"\xfb", b"\x1c", b"\x1c\x12", b"\xff", b"\xff\x00", b"\xff\x00\x00\x01"))
        elif kind == "outside":
            s = rng.choice("lg")
            idx = rng.choice((self.n[s], -1, self.n[s] + rng.randint(1, 50)))
            t += [self.index(idx - K.bias(self.n[s])), _OPB["callsubr" if s == "l" else "callgsubr"]]
        elif kind == "mask":
            more = rng.randint(1, 12)
            if self.cff2:                                            # (no failure in CFF2: the stream ends)
                t += self.args(2 * more, p_blend=0.0) + [self.mask(more, short=1)]
                return t
            t += self.args(2 * more) + [_OPB["hstemhm"]]
            t.append(self.mask(more, short=1))
            return t
        elif kind == "overflow":
            t += self.args(49 if not self.cff2 else 514, p_blend=0.0) + [_OPB["hlineto"]]
            self.no_calls = True
        elif kind == "depth":
            self.levels = 11
        elif kind == "ends":
            t.append(_OPB[rng.choice(("return", "endchar"))])
        elif kind == "second_width":
            mv = rng.choice(tuple(_MOVES))
            t += self.args(_MOVES[mv] + 1) + [_OPB[mv]]
        self.contours(t, stems, 1, (1, 2), 0.0)
        if not self.cff2 and cut is None:
            t.append(_OPB["endchar"])
        if kind == "after_endchar":
            t += rng.choice(([self.num()], [self.num(), _OPB["hlineto"]], [_OPB["endchar"]], [_OPB["return"]]))
        if cut is not None:
            t.append(cut)
        return t

    def outline(self, toks, levels):
        """move a random span of the tokens into a subroutine, and spans of that span further down, `levels` deep"""
        rng = self.rng
        if levels == 0 or not toks:
            return toks
        a = rng.randrange(len(toks))
        b = rng.randint(a + 1, len(toks)) if rng.random() < 0.8 else len(toks)
        body = self.outline(toks[a:b], levels - 1)
        if not self.cff2 and body[-1] != _OPB["endchar"] and rng.random() < 0.8:
            body = body + [_OPB["return"]]
        s = rng.choice("lg")
        blob = b"".join(body)
        idx = self.known.get((s, blob))
        if idx is None:
            if not self.free[s]:
                s = "g" if s == "l" else "l"
            if not self.free[s]:
                return toks
            idx = self.free[s].pop(0)
            self.subrs[s][idx] = blob
            self.known[(s, blob)] = idx
        return toks[:a] + [self.index(idx - K.bias(self.n[s])), _OPB["callsubr" if s == "l" else "callgsubr"]] + toks[b:]

    def glyph(self, kind):
        rng = self.rng
        self.mode = "inexact" if rng.random() < 0.3 else "exact"
        self.width = not self.cff2 and rng.random() < 0.5
        self.set_index = rng.choice((K2.K4, K2.K4, K2.K4, K2.K2, K2.K2, K2.K1, K2.K1, K2.K64, K2.K64, K2.K0))
        self.k = K2.REGIONS_OF[self.set_index]
        self.no_calls, self.levels = False, rng.choice((0, 0, 0, 1, 1, 2, 3, rng.randint(4, 10)))
        if kind == "empty":
            return b""
        toks = self.failing() if kind == "fail" else self.normal(long=kind == "long")
        if not self.no_calls:
            # (several spans side by side, then the nest)
            for _ in range(rng.choice((0, 0, 1, 2)) if self.levels else 0):
                toks = self.outline(toks, 1)
            toks = self.outline(toks, self.levels)
        return b"".join(toks)

    def sets(self):
        filler = b"" if self.cff2 else K.RET
        return ([self.subrs[s].get(i, filler) for i in range(self.n[s])] for s in "lg")


def _face_of(name, glyphs, b, cff2):
    loc, glo = b.sets()
    # (the five usable sets of the hand-written kit: fontTools cannot read a store with the two that are not)
    return K2.Face(name, glyphs, glo, loc, list(K2.SETS[:5])) if cff2 else K.Face(name, glyphs, glo, [loc])


def run(desc, gid, cff2, sets=None, budget=MAX_RUN_TOKENS, trace=None, interpret=None):
    fn = interpret or (K2.interpret if cff2 else K.interpret)
    return fn(desc, gid, sets, budget, trace) if cff2 else fn(desc, gid, budget, trace)


def face(seed, cff2, n_glyphs=N_GLYPHS):
    """a face of n_glyphs random programs (glyph id 0 is .notdef).  Every eighth seed's face (seed % 8 == 2) of at least 128 glyph
    ids holds a wave (glyph ids 64 .. 127) of 63 empty charstrings around one long one"""
    rng = random.Random(f"{'cff2' if cff2 else 'cff'}/{seed}/{n_glyphs}")
    b = _Builder(rng, cff2, rng.choice(_SET_SIZES), rng.choice(_SET_SIZES))
    wave = {}
    if seed % 8 == 2 and n_glyphs >= 128:
        wave = {g: "empty" for g in range(64, 128)}
        wave[64 + rng.randrange(64)] = "long"
    glyphs = [(".notdef", K2.NOTDEF if cff2 else K.NOTDEF)]
    for g in range(1, n_glyphs):
        for _ in range(50):
            kind = wave.get(g) or rng.choices(("normal", "fail", "empty"), (84, 13, 3))[0]
            saved = ({s: dict(v) for s, v in b.subrs.items()}, {s: list(v) for s, v in b.free.items()}, dict(b.known))
            cs = b.glyph(kind)
            o = run(_face_of("one", [("g", cs)], b, cff2).desc(), 0, cff2)
            if o.end not in ("budget", "seac"):
                break
            b.subrs, b.free, b.known = saved
        else:
            raise AssertionError("no program within the token cap")
        glyphs.append((f"g{g}", cs))
    return _face_of(f"fuzz{'2' if cff2 else ''}_{seed}_{n_glyphs}", glyphs, b, cff2)


# ---- what a run reached --------------------------------------------------------------------------------------------------------

_PATH_OPS = {5: "rlineto", 6: "hlineto", 7: "vlineto", 8: "rrcurveto", 24: "rcurveline", 25: "rlinecurve", 26: "vvcurveto", 27: "hhcurveto",
             30: "vhcurveto", 31: "hvcurveto", (12, 34): "hflex", (12, 35): "flex", (12, 36): "hflex1", (12, 37): "flex1"}
_CLEARING = {1: "hstem", 3: "vstem", 18: "hstemhm", 23: "vstemhm", 19: "hintmask", 20: "cntrmask", 21: "rmoveto", 22: "hmoveto", 4: "vmoveto",
             14: "endchar"}


def _forms(name, sp):
    if name in ("rlineto", "rrcurveto"):
        return [f"{name}_{'1' if sp == (2 if name == 'rlineto' else 6) else 'n'}"]
    if name in ("hlineto", "vlineto"):
        return [f"{name}_{'odd' if sp & 1 else 'even'}"]
    if name == "rcurveline":
        return [f"rcurveline_{'1' if sp == 8 else 'n'}"]
    if name == "rlinecurve":
        return [f"rlinecurve_{'1' if sp == 8 else 'n'}"]
    if name in ("vvcurveto", "hhcurveto"):
        return [f"{name}_{'lead' if sp & 1 else 'plain'}_{'1' if sp < 8 else 'n'}"]
    if name in ("hvcurveto", "vhcurveto"):
        return [f"{name}_{'tail' if sp & 1 else 'plain'}_{'odd' if (sp >> 2) & 1 else 'even'}"]
    return [name]


def features(desc, gid, cff2, sets=None):
    """(the outcome, the set of FEATURES names the run reached).  Everything is read off the interpreter's state at each token it
    executes; what a token did counts only if the run went on behind it (or ended well with it)"""
    n_sets = {10: len(desc["lsubr_off"]) - 1 if cff2 else None, 29: len(desc["gsubr_off"]) - 1}
    if not cff2:
        fd = 0 if desc.get("fd_of") is None else int(desc["fd_of"][gid])
        n_sets[10] = int(desc["lsubr_first"][fd + 1]) - int(desc["lsubr_first"][fd])
    limit = K2.MAX_OPERANDS2 if cff2 else K.MAX_OPERANDS
    done, pending, pushed_at, last, calls = set(), [], [], [None], [0]

    def trace(op, data, pos, end, stack, depth, st):
        done.update(pending)
        del pending[:]
        del pushed_at[len(stack):]
        sp, f = len(stack), pending.append
        last[0] = why = None
        if isinstance(op, int) and (op >= 32 or op == 28):
            size = 2 if op == 28 else 0 if op <= 246 else 1 if op <= 254 else 4
            if end - pos < size:
                why = "fail_truncated_operand"
            elif sp >= limit:
                why = "fail_stack_overflow"
                done.add("stack_past_limit_attempted")
            else:
                pushed_at.append(depth)
                if op == 28:
                    v = struct.unpack(">h", data[pos:pos + 2])[0]
                    f("operand_28")
                    if -1131 <= v <= 1131:
                        f("operand_28_shorter_would_do")
                elif op == 255:
                    v = struct.unpack(">i", data[pos:pos + 4])[0]
                    f("operand_255_fraction" if v & 0xFFFF else "operand_255_whole")
                else:
                    f("operand_1_byte" if op <= 246 else "operand_2_bytes_positive" if op <= 250 else "operand_2_bytes_negative")
                if sp + 1 == limit:
                    f("stack_at_limit")
                if cff2 and 40 <= sp + 1 <= 60:
                    f("stack_40_to_60")
                if cff2 and sp + 1 > 500:
                    f("stack_above_500")
            last[0] = why
            return
        if op == 12:
            if pos >= end:
                last[0] = "fail_underflow"
            return
        name = _PATH_OPS.get(op)
        if name is not None:
            if not st["has_move"]:
                why = "fail_path_before_move"
            else:
                why = "fail_underflow"                 # (if it fails at all: an operand count no form has)
                for form in _forms(name, sp):
                    f(form)
                if cff2 and sp > K2.WINDOW:
                    f("operands_read_above_the_window")
        elif op in _CLEARING and not (cff2 and op == 14):
            cname, why = _CLEARING[op], "fail_underflow"
            if op in (1, 3, 18, 23):
                f(f"stem_{cname}")
            if not cff2:
                odd = (sp - _MOVES.get(cname, 0)) & 1 if cname in _MOVES else sp & 1
                if op == 14:
                    why = "fail_data_after_endchar"
                if not st["width"]:
                    f(f"width_{'on' if odd else 'absent'}_{cname}")
            if op in (19, 20):
                total = st["stems"] + ((sp - (sp & 1)) >> 1)
                n = (total + 7) >> 3
                if sp >= 2:
                    f("mask_implicit_vstem")
                if n > end - pos:
                    why = "fail_mask_past_end"
                    if cff2:
                        f("end_mask_past_end" if depth == 0 else "mask_past_end_in_subr")
                else:
                    if n in (1, 2, 3, 12, 13):
                        f(f"mask_bytes_{n}")
                    if total in (8, 9, 16, 17, 96, 97):
                        f(f"mask_stems_{total}")
        elif op in (10, 29):
            why = "fail_underflow"
            if sp > 0:
                n = n_sets[op]
                v = stack[-1]
                idx = int(v) + K.bias(n)
                if depth >= K.MAX_DEPTH:
                    why = "fail_depth_11"
                elif float(v) == int(v) and not 0 <= idx < n:
                    why = "fail_call_outside_set"
                else:
                    calls[0] += 1
                    f(f"call_depth_{depth + 1}")
                    f("call_local" if op == 10 else "call_global")
                    f(f"call_set_{'below' if n < 1240 else 'from'}_1240")
                    if int(v) in (0, -107):
                        f(f"call_operand_{int(v)}")
                    if idx == n - 1:
                        f("call_last_index")
        elif cff2 and op == 15:
            why = "fail_underflow"
            if sp == 1:
                f(f"vsindex_{int(stack[0])}")
        elif cff2 and op == 16:
            why = "fail_underflow"
            if sp > 0 and stack[-1] >= 0:
                n, k = int(stack[-1]), len(st["scalars"])
                start = sp - 1 - n * (k + 1)
                if start >= 0 and n >= 1:
                    f(f"blend_regions_{k}")
                    f("blend_1_value" if n == 1 else "blend_n_values")
                    if k and start < K2.WINDOW < sp - 1:
                        f("blend_astride_the_window")
                    if k and start >= K2.WINDOW:
                        f("blend_above_the_window")
        elif op == 11 and not cff2:
            pass
        else:
            why = "fail_return_or_endchar" if cff2 and op in (11, 14) else "fail_underflow"
        if name is not None or op in _CLEARING:
            if sp and len(set(pushed_at[:sp])) > 1:
                f("operands_across_a_subroutine_boundary")
        last[0] = why

    o = run(desc, gid, cff2, sets, trace=trace)
    if o.end == "fail":
        if last[0]:
            done.add(last[0])
    else:
        done.update(pending)
        if not calls[0]:
            done.add("call_depth_0")
        if cff2 and "end_mask_past_end" not in done:
            done.add("end_with_the_data")
    if not cff2 and o.end in ("end", "return"):
        done.add("end_without_endchar")
    return o, done


def _feature_table():
    both = ["operand_1_byte", "operand_2_bytes_positive", "operand_2_bytes_negative", "operand_28", "operand_28_shorter_would_do",
            "operand_255_fraction", "operand_255_whole", "stack_at_limit", "stack_past_limit_attempted", "mask_implicit_vstem",
            "operands_across_a_subroutine_boundary", "call_local", "call_global", "call_set_below_1240", "call_set_from_1240",
            "call_operand_0", "call_operand_-107", "call_last_index", "fail_underflow", "fail_path_before_move", "fail_truncated_operand",
            "fail_call_outside_set", "fail_stack_overflow", "fail_depth_11"]
    both += [f"call_depth_{d}" for d in range(11)] + [f"stem_{s}" for s in _STEMS]
    both += [f"mask_bytes_{n}" for n in (1, 2, 3, 12, 13)] + [f"mask_stems_{n}" for n in (8, 9, 16, 17, 96, 97)]
    for name in ("rlineto", "rrcurveto", "rcurveline", "rlinecurve"):
        both += [f"{name}_1", f"{name}_n"]
    for name in ("hlineto", "vlineto"):
        both += [f"{name}_odd", f"{name}_even"]
    for name in ("vvcurveto", "hhcurveto"):
        both += [f"{name}_{a}_{b}" for a in ("lead", "plain") for b in ("1", "n")]
    for name in ("hvcurveto", "vhcurveto"):
        both += [f"{name}_{a}_{b}" for a in ("tail", "plain") for b in ("odd", "even")]
    both += ["flex", "hflex", "hflex1", "flex1"]
    cff = both + [f"width_{w}_{c}" for w in ("on", "absent") for c in _CLEARING.values()] + ["fail_mask_past_end", "fail_data_after_endchar",
                                                                                              "end_without_endchar"]
    cff2 = both + [f"blend_regions_{k}" for k in (0, 1, 2, 4, 64)] + [f"vsindex_{s}" for s in (0, 1, 2, 3, 4)]
    cff2 += ["blend_1_value", "blend_n_values", "blend_astride_the_window", "blend_above_the_window", "operands_read_above_the_window",
             "stack_40_to_60", "stack_above_500", "end_with_the_data", "end_mask_past_end", "mask_past_end_in_subr", "fail_return_or_endchar"]
    return {"cff": cff, "cff2": cff2}


FEATURES = _feature_table()      # what a corpus must reach, per decoder, on at least three glyphs of different faces


# ---- numbers that count their own roundings ------------------------------------------------------------------------------------

class Tracked(float):
    """an f32 value (held in a float) with n, the number of f32 roundings on the way to it that changed a value, and mag, the
    largest magnitude on that way: a reader that computes the same value in f64 from the same inputs is within
    n x half an ulp of mag (bound()), and equal where n is 0"""

    def __new__(cls, v, n=0, mag=0.0):
        self = float.__new__(cls, v)
        self.n, self.mag = n, max(mag, abs(float(v)))
        return self

    def bound(self):
        return 0.0 if self.n == 0 else self.n * 2.0 ** (math.frexp(self.mag)[1] - 1 - 24)


def tracked(v):
    """stands in for numpy.float32 in an interpreter"""
    if isinstance(v, Tracked):
        return v
    x = float(np.float32(v))
    return Tracked(x, 0 if x == float(v) else 1)


def tracked_fixed(raw):
    """a 16.16 operand: one rounding where f32 cannot hold the 32-bit integer (its magnitude is the operand's, not the integer's)"""
    x = float(np.float32(raw)) / 65536.0
    return Tracked(x, 0 if x * 65536.0 == raw else 1)


def _binary(fn, swap=False):
    def op(a, b):
        if swap:
            a, b = b, a
        with np.errstate(all="ignore"):
            exact = fn(float(a), float(b))
            r = float(np.float32(exact))
        n = getattr(a, "n", 0) + getattr(b, "n", 0) + (0 if r == exact else 1)
        return Tracked(r, n, max(getattr(a, "mag", abs(float(a))), getattr(b, "mag", abs(float(b)))))
    return op


for _name, _fn in (("add", operator.add), ("sub", operator.sub), ("mul", operator.mul), ("truediv", operator.truediv)):
    setattr(Tracked, f"__{_name}__", _binary(_fn))
    setattr(Tracked, f"__r{_name}__", _binary(_fn, swap=True))
Tracked.__neg__ = lambda a: Tracked(-float(a), a.n, a.mag)


def variant(fn, *swaps, **names):
    """fn with pieces of its source replaced ((old, new) pairs, each old piece exactly once in it) and run over the module's names
    and `names`"""
    src = inspect.getsource(fn)
    for old, new in swaps:
        assert src.count(old) == 1, (fn.__name__, old, src.count(old))
        src = src.replace(old, new)
    ns = dict(inspect.getmodule(fn).__dict__, **names)
    exec(compile(src, f"<{fn.__name__} variant>", "exec"), ns)
    return ns[fn.__name__]


_F32 = ("    f32 = np.float32\n", "    f32 = tracked\n")
_FIXED = ("v = f32(struct.unpack(\">i\", data[pos:pos + 4])[0]) / f32(65536.0)", "v = tracked_fixed(struct.unpack(\">i\", data[pos:pos + 4])[0])")
_TRACKED = {False: variant(K.interpret, _F32, _FIXED, tracked=tracked, tracked_fixed=tracked_fixed),
            True: variant(K2.interpret, _F32, _FIXED, ("np.asarray(sets[\"factors\"], np.float32)", "[tracked(v) for v in np.asarray(sets[\"factors\"], np.float32)]"),
                          tracked=tracked, tracked_fixed=tracked_fixed)}


def tracked_run(desc, gid, cff2, sets=None):
    """the outcome with Tracked coordinates"""
    o = run(desc, gid, cff2, sets, interpret=_TRACKED[cff2])
    assert all(isinstance(v, Tracked) for v in o.coords)
    return o


# ---- one rule broken each ------------------------------------------------------------------------------------------------------

def _mutants():
    out = []
    both = [
        ("hvcurveto_trailing_operand_dropped", ("last = stack[i + 4] if left == 5 else f32(0)", "last = f32(0)")),
        ("mask_length_floor", ("need((st[\"stems\"] + 7) >> 3 <= end - pos)\n                pos += (st[\"stems\"] + 7) >> 3",
                               "need(st[\"stems\"] >> 3 <= end - pos)\n                pos += st[\"stems\"] >> 3"),
         ("pos = min(pos + ((st[\"stems\"] + 7) >> 3), end)", "pos = min(pos + (st[\"stems\"] >> 3), end)")),
        ("implicit_vstem_not_counted", ("                st[\"stems\"] += n >> 1\n                need(", "                need("),
         ("                st[\"stems\"] += n >> 1\n                pos = min", "                pos = min")),
        ("stack_kept_after_a_stem", ("                st[\"stems\"] += n >> 1\n                stack.clear()\n", "                st[\"stems\"] += n >> 1\n"),
         ("                st[\"stems\"] += sp >> 1             # (no width: an odd operand is simply left over)\n                stack.clear()\n",
          "                st[\"stems\"] += sp >> 1\n")),
        ("hhcurveto_lead_operand_on_x", ("                    else:\n                        st[\"y\"] = st[\"y\"] + stack[0]\n                    i = 1",
                                         "                    else:\n                        st[\"x\"] = st[\"x\"] + stack[0]\n                    i = 1")),
        ("flex1_compares_the_wrong_way", ("if abs(x2 - x0) > abs(y2 - y0):", "if abs(x2 - x0) >= abs(y2 - y0):")),
        ("rlinecurve_line_count_one_short", ("for i in range(0, sp - 6, 2):", "for i in range(0, sp - 8, 2):")),
    ]
    for name, first, *second in both:
        out.append((name, "cff", variant(K.interpret, first)))
        out.append((name, "cff2", variant(K2.interpret, second[0] if second else first)))
    out.append(("bias_off_by_one_at_1240", "cff", variant(K.interpret, ("idx = int(fidx) + bias(n)", "idx = int(fidx) + (107 if n <= 1240 else bias(n))"))))
    out.append(("bias_off_by_one_at_1240", "cff2", variant(K2.interpret, ("idx = int(fidx) + bias(n)", "idx = int(fidx) + (107 if n <= 1240 else bias(n))"))))
    out.append(("width_parity_ignored", "cff", variant(K.interpret, ("                if (n & 1) and not st[\"width\"]:\n", "                if not st[\"width\"]:\n"))))
    out.append(("width_taken_twice", "cff", variant(K.interpret, ("if sp == want + 1 and not st[\"width\"]:", "if sp == want + 1:"))))
    out.append(("stack_limit_49", "cff", variant(K.interpret, ("need(len(stack) < MAX_OPERANDS)", "need(len(stack) <= MAX_OPERANDS)"))))
    out.append(("depth_limit_11", "cff", variant(K.interpret, ("need(sp > 0 and depth < MAX_DEPTH)", "need(sp > 0 and depth <= MAX_DEPTH)"))))
    out.append(("blend_folds_in_reverse_order", "cff2", variant(K2.interpret, ("for i in range(n - 1, -1, -1):", "for i in range(n):"))))
    out.append(("blend_factors_in_reverse_order", "cff2", variant(K2.interpret, ("scalars[k - j - 1]", "scalars[j]"))))
    out.append(("window_slot_48_aliased_to_47", "cff2", variant(
        K2.interpret, ("                need(len(stack) < MAX_OPERANDS2)\n                stack.append(v)\n",
                       "                need(len(stack) < MAX_OPERANDS2)\n                stack.append(v)\n                if len(stack) == WINDOW + 1:\n"
                       "                    stack[WINDOW - 1] = v\n"))))
    out.append(("vsindex_ignored", "cff2", variant(K2.interpret, ("need(select(int(v)))", "need(int(v) < len(set_ok))"))))
    out.append(("stack_limit_514", "cff2", variant(K2.interpret, ("need(len(stack) < MAX_OPERANDS2)", "need(len(stack) <= MAX_OPERANDS2)"))))
    return out


MUTANTS = _mutants()             # (rule, decoder, interpret): every one must disagree with the host reader somewhere in a corpus


# ---- fontTools' own interpreter -------------------------------------------------------------------------------------------------

# what fontTools' interpreter cannot read although the rules allow it: it asserts that a mask's bytes are all there, and it takes
# a selected set of no regions for "no set selected yet" (the default set's region count stands in).  A glyph that reached one of
# these is left out of the comparison with fontTools, like the glyphs that fail
FONTTOOLS_BLIND = ("end_mask_past_end", "mask_past_end_in_subr", "blend_regions_0")


def fonttools_commands(font_bytes, location=None, normalized=False):
    """[(kinds, [coordinates as floats])] per glyph id, drawn by fontTools' T2 interpreter (CFF2: with its blender at the
    location); None where it raises"""
    import io
    from fontTools.pens.recordingPen import RecordingPen
    from fontTools.ttLib import TTFont
    f = TTFont(io.BytesIO(font_bytes))
    gs = f.getGlyphSet(location=location, normalized=normalized) if location is not None else f.getGlyphSet()
    out = []
    for name in f.getGlyphOrder():
        pen = RecordingPen()
        try:
            gs[name].draw(pen)
        except Exception:
            out.append(None)
            continue
        kinds, coords = [], []
        for what, pts in pen.value:
            kinds.append({"moveTo": K.M, "lineTo": K.L, "curveTo": K.C, "closePath": K.Z, "endPath": K.Z}[what])
            coords += [float(v) for p in pts for v in p]
        out.append((kinds, coords))
    return out


# ---- the comparisons the tests and tools/fuzz_decoders.py share --------------------------------------------------------------------

POSITIONS2 = (None, [8192], [5461])      # of a CFF2 face: the default position, one whose factors are exact, one whose are not


def host_views(vg, font, cff2, coords=None):
    """(the description for the device, the host reader's command table) of the face, a CFF2 face placed at coords if given"""
    mgr = vg.FontManager(False)
    fid = mgr.add_font_data("Fuzz", font) if coords is None else mgr.add_font_instance_normalized("Fuzz", font, list(coords))
    return (mgr.charstring2_font_desc if cff2 else mgr.charstring_font_desc)(fid, 0), mgr.command_font_desc(fid, 0)


def commands_of(o):
    return bytes(o.kinds), np.array(o.coords, np.float32).tobytes()


def first_difference(name, desc, host, cff2, interpret=None):
    """None where the host reader's table is the interpreter's for every glyph id, bit for bit; else a line that names the glyph
    id and the first differing record"""
    for g in range(len(desc["cs_off"]) - 1):
        o = run(desc, g, cff2, interpret=interpret)
        if K.glyph_commands(host, g) != commands_of(o):
            kinds, coords = K.glyph_commands(host, g)
            a, b = _records(kinds, np.frombuffer(coords, np.float32)), _records(bytes(o.kinds), np.array(o.coords, np.float32))
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return f"{name}: glyph id {g} (ends: {o.end}), command {at}: host {a[at:at + 1]}, interpreter {b[at:at + 1]}"
    return None


_FLOATS = {K.M: 2, K.L: 2, K.C: 6, K.Z: 0, 2: 4}


def _records(kinds, coords):
    out, at = [], 0
    for kind in kinds:
        out.append((kind, coords[at:at + _FLOATS[kind]].tobytes().hex()))
        at += _FLOATS[kind]
    return out
