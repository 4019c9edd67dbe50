"""Hand-written `loca` + `glyf` tables that sit on the edges of the composite walk (csrc/host/ttf_face.cpp, GlyfWalker::walk; on
the device csrc/glyf_table_kernels.hip), and a strict Python restatement of the resident form they make.  A plain helper module:
tests/test_font_tables_desc_host.py pins the restatement to the host's table (Face::resident_table), the GPU tests compare the
device-built font with vgsdf_font_create of the restated arrays.

restate(tables) gives the layout vgsdf_font_create_tables documents (include/vgsdf.h): the leaves in the host's order, every
glyph id's own simple entry stored in glyph-id order at byte_at[glyph id] — or REFUSED_BOUNDS (where the host's table is not ok)
or REFUSED_BUDGET (a glyph id past VGSDF_GLYF_MAX_COMPONENTS component records; the host has no such budget).

A Forest collects named glyphs; composites name their children by glyph name (or by a literal glyph id), so the cases can stand
alone or side by side in one font, in any order."""
import io
from collections import namedtuple

import numpy as np

from glyf_edge_entries import entry, plain, coords_for

# csrc/glyf_table_limits.h
MAX_DEPTH, MAX_ENTRY, MAX_COMPONENTS = 32, 32 * 1024, 1 << 20
MAX_LEAVES, MAX_GLYPH_SLOTS, MAX_BYTES, MAX_SLOT_SUM = 1 << 22, 1 << 26, (1 << 32) - 4, (1 << 32) - 1
REFUSED_BOUNDS, REFUSED_BUDGET = "refused: bounds", "refused: budget"

PART_DTYPE = np.dtype([("byte_off", "<u4"), ("byte_len", "<u4"), ("cmd_at", "<u4"), ("cmd_cap", "<u4"), ("n_contours", "<u4"),
                       ("plain", "<u4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("d", "<f4"), ("e", "<f4"), ("f", "<f4")])

Tables = namedtuple("Tables", "loca glyf num_glyphs loca_entries loca_long")

ARGS_WORDS, ARGS_XY, SCALE, MORE, XY_SCALE, TWO_BY_TWO = 0x0001, 0x0002, 0x0008, 0x0020, 0x0040, 0x0080


def desc(t):
    """the dict SdfContext.font_create_tables takes"""
    return {"loca": t.loca, "glyf": t.glyf, "num_glyphs": t.num_glyphs, "loca_entries": t.loca_entries, "loca_long": t.loca_long}


# ---- the strict restatement ----

def _u16(b, at):
    return (b[at] << 8) | b[at + 1]


def _i16(b, at):
    v = _u16(b, at)
    return v - 0x10000 if v & 0x8000 else v


def _i8(v):
    return v - 0x100 if v & 0x80 else v


F32 = np.float32
IDENTITY = (F32(1), F32(0), F32(0), F32(1), F32(0), F32(0))


def _then(p, k):
    """Affine::then in f32: every product and every sum rounded, in the written order"""
    a, b, c, d, e, f = p
    ka, kb, kc, kd, ke, kf = k
    return (a * ka + c * kb, b * ka + d * kb, a * kc + c * kd, b * kc + d * kd, a * ke + c * kf + e, b * ke + d * kf + f)


def _f2dot14(b, at):
    return F32(_i16(b, at)) / F32(16384.0)


FAIL, NOTHING = "fail", "nothing"


def measure(glyf, at, end, nc):
    """PartShape::measure over the entry's body glyf[at:end] -> FAIL, NOTHING or (n_points, cur, ends, arrays)"""
    size = end - at
    if nc * 2 > size:
        return FAIL
    last = _u16(glyf, at + (nc - 1) * 2)
    if last == 0xFFFF:
        return FAIL
    n_points = last + 1
    if n_points == 1:
        return NOTHING
    cur = nc * 2
    if size - cur < 2:
        return FAIL
    cur += 2 + _u16(glyf, at + cur)
    if cur > size:
        return FAIL
    fits = nc * 2 + (size - cur) <= MAX_ENTRY
    return n_points, cur, (nc * 2 if fits else 0), (size - cur if fits else 0)


class _Refused(Exception):
    pass


def glyph_range(t, gid):
    """Face::glyph_data"""
    if not t.loca or not t.glyf or gid == 0xFFFF or gid + 1 >= t.loca_entries:
        return None
    if t.loca_long:
        a = int.from_bytes(t.loca[4 * gid:4 * gid + 4], "big")
        b = int.from_bytes(t.loca[4 * gid + 4:4 * gid + 8], "big")
    else:
        a, b = 2 * _u16(t.loca, 2 * gid), 2 * _u16(t.loca, 2 * gid + 2)
    if a >= b or b > len(t.glyf):
        return None
    return a, b


_RESTATED = {}
_WHOLE = 1 << 20


class _Leaves:
    """the leaves so far: records appended one by one or array by array"""

    def __init__(self):
        self.n, self.chunks, self.pending = 0, [], []

    def __len__(self):
        return self.n

    def append(self, leaf):
        self.pending.append(leaf)
        self.n += 1

    def extend(self, arr):
        self._flush()
        self.chunks.append(arr)
        self.n += len(arr)

    def _flush(self):
        if self.pending:
            self.chunks.append(np.array(self.pending, dtype=PART_DTYPE).reshape(-1))
            self.pending = []

    def tail(self, first):
        """leaves[first:] as one array"""
        self._flush()
        if len(self.chunks) > 1:
            self.chunks = [np.concatenate(self.chunks)]
        return self.chunks[0][first:] if self.chunks else np.zeros(0, dtype=PART_DTYPE)


def restate(t):
    """-> {leaf_off, leaves, bytes, slots, records} or REFUSED_BOUNDS / REFUSED_BUDGET.  records: the component records each glyph id read"""
    if t in _RESTATED:
        return _RESTATED[t]
    assert t.num_glyphs <= 0xFFFF and t.loca_long in (0, 1) and t.loca_entries * (4 if t.loca_long else 2) <= len(t.loca)
    glyf, n = t.glyf, t.num_glyphs
    # the bytes, in glyph-id order
    store, byte_at = bytearray(), []
    for gid in range(n):
        byte_at.append(len(store))
        r = glyph_range(t, gid)
        if r is None or r[1] - r[0] < 10:
            continue
        a, b = r
        nc = _i16(glyf, a)
        if nc <= 0:
            continue
        m = measure(glyf, a + 10, b, nc)
        if m in (FAIL, NOTHING):
            continue
        _, cur, ends, arrays = m
        store += glyf[a + 10:a + 10 + ends] + glyf[a + 10 + cur:a + 10 + cur + arrays]
        store += b"\0" * (-len(store) % 4)
    leaves, leaf_off, slots_of, records_of = _Leaves(), [0], [], []
    state = {"slots": 0, "records": 0, "deep": 0}
    # A composite child that has been walked once, whole and without a failure, is REPLAYED where it is named again — but only
    # where that cannot change a bit: the transform it is entered with and every leaf below it are pure translations by whole
    # numbers below 2^20, so every product is by 1 or 0 and every sum exact, whatever the order Affine::then takes them in; and it
    # ends above depth 32 again.  Everything else is walked record by record.  glyph id -> (levels below its entry, records, leaves
    # with cmd_at, e and f counted from its entry)
    memo = {}

    def plain_shift(tr):
        a, b, c, d, e, f = tr
        return a == 1 and b == 0 and c == 0 and d == 1 and abs(e) < _WHOLE and abs(f) < _WHOLE and e == int(e) and f == int(f)

    def replay(child, depth, tr):
        """the leaves of memo[child] entered at `depth` with `tr`; False: not replayed"""
        if child not in memo or not plain_shift(tr) or depth + memo[child][0] >= MAX_DEPTH:
            return False
        _, records, sub = memo[child]
        state["records"] += records
        if state["records"] > MAX_COMPONENTS:
            raise _Refused(REFUSED_BUDGET)
        if state["slots"] + int(sub["cmd_at"][-1]) + int(sub["cmd_cap"][-1]) > MAX_GLYPH_SLOTS or len(leaves) + len(sub) > MAX_LEAVES:
            raise _Refused(REFUSED_BOUNDS)
        out = sub.copy()
        out["cmd_at"] += np.uint32(state["slots"])
        out["e"] = tr[0] * sub["e"] + tr[2] * sub["f"] + tr[4]       # Affine::then of a pure shift, as written
        out["f"] = tr[1] * sub["e"] + tr[3] * sub["f"] + tr[5]
        out["plain"] = ((out["e"] == 0) & (out["f"] == 0)).astype(np.uint32)
        leaves.extend(out)
        state["slots"] += int(sub["cmd_at"][-1]) + int(sub["cmd_cap"][-1])
        state["deep"] = max(state["deep"], depth + memo[child][0])
        return True

    def remember(child, depth, tr, first_leaf, first_slot, first_record):
        """after a walk of `child` at `depth` that returned True"""
        if child in memo or not plain_shift(tr) or len(leaves) - first_leaf < 2:
            return
        sub = leaves.tail(first_leaf).copy()
        if not ((sub["a"] == 1) & (sub["b"] == 0) & (sub["c"] == 0) & (sub["d"] == 1)).all():
            return
        sub["cmd_at"] -= np.uint32(first_slot)
        sub["e"] -= tr[4]
        sub["f"] -= tr[5]
        if not ((np.abs(sub["e"]) < _WHOLE) & (np.abs(sub["f"]) < _WHOLE) & (sub["e"] == np.floor(sub["e"])) & (sub["f"] == np.floor(sub["f"]))).all():
            return
        memo[child] = (state["deep"] - depth, state["records"] - first_record, sub)

    def walk(a, b, depth, tr, gid):
        if depth >= MAX_DEPTH or b - a < 2:
            return False
        state["deep"] = max(state["deep"], depth)
        nc = _i16(glyf, a)
        if nc > 0:
            if b - a < 10:
                return False
            m = measure(glyf, a + 10, b, nc)
            if m == FAIL:
                return False
            if m == NOTHING:
                return True
            n_points, _, ends, arrays = m
            cap = n_points + 2 * nc
            if state["slots"] + cap > MAX_GLYPH_SLOTS or len(leaves) >= MAX_LEAVES:
                raise _Refused(REFUSED_BOUNDS)
            leaves.append((byte_at[gid], ends + arrays, state["slots"], cap, nc, 1 if tr == IDENTITY else 0) + tr)
            state["slots"] += cap
            return True
        if nc == 0 or b - a < 10:
            return nc == 0
        p = a + 10
        while True:
            if b - p < 4:
                break
            fl, child = _u16(glyf, p), _u16(glyf, p + 2)
            p += 4
            state["records"] += 1
            if state["records"] > MAX_COMPONENTS:
                raise _Refused(REFUSED_BUDGET)
            ka, kb, kc, kd, ke, kf = IDENTITY
            if fl & ARGS_XY:
                if fl & ARGS_WORDS:
                    if b - p < 4:
                        break
                    ke, kf = F32(_i16(glyf, p)), F32(_i16(glyf, p + 2))
                    p += 4
                else:
                    if b - p < 2:
                        break
                    ke, kf = F32(_i8(glyf[p])), F32(_i8(glyf[p + 1]))
                    p += 2
            if fl & TWO_BY_TWO:
                if b - p < 8:
                    break
                ka, kb, kc, kd = _f2dot14(glyf, p), _f2dot14(glyf, p + 2), _f2dot14(glyf, p + 4), _f2dot14(glyf, p + 6)
                p += 8
            elif fl & XY_SCALE:
                if b - p < 4:
                    break
                ka, kd = _f2dot14(glyf, p), _f2dot14(glyf, p + 2)
                p += 4
            elif fl & SCALE:
                if b - p < 2:
                    break
                ka = kd = _f2dot14(glyf, p)
                p += 2
            r = glyph_range(t, child)
            if r is not None:
                below = _then(tr, (ka, kb, kc, kd, ke, kf))
                if not replay(child, depth + 1, below):
                    mark, deep = (len(leaves), state["slots"], state["records"]), state["deep"]
                    state["deep"] = depth + 1
                    ok = walk(r[0], r[1], depth + 1, below, child)
                    if ok:
                        remember(child, depth + 1, below, *mark)
                    state["deep"] = max(state["deep"], deep)
                    if not ok:
                        return False
            if not fl & MORE:
                break
        return True

    slot_sum = 0
    out = None
    try:
        with np.errstate(all="ignore"):
            for gid in range(n):
                state["slots"], state["records"] = 0, 0
                r = glyph_range(t, gid)
                if r is not None:
                    walk(r[0], r[1], 0, IDENTITY, gid)
                slot_sum += state["slots"]
                if slot_sum > MAX_SLOT_SUM:
                    raise _Refused(REFUSED_BOUNDS)
                leaf_off.append(len(leaves))
                slots_of.append(state["slots"])
                records_of.append(state["records"])
        if len(store) > MAX_BYTES:
            raise _Refused(REFUSED_BOUNDS)
    except _Refused as why:
        out = str(why)
    if out is None:
        out = {"leaf_off": np.array(leaf_off, dtype=np.uint32), "leaves": leaves.tail(0),
               "bytes": np.frombuffer(bytes(store), dtype=np.uint8), "slots": np.array(slots_of, dtype=np.uint32),
               "records": records_of, "byte_at": np.array(byte_at + [len(store)], dtype=np.uint32)}
    _RESTATED[t] = out
    return out


# ---- building entries ----

def i16(v):
    return int(v).to_bytes(2, "big", signed=True)


def f2(v):
    """F2Dot14 of a value in [-2, 2)"""
    return i16(round(v * 16384))


def simple(n_points=4, n_contours=1, instructions=b"", trailing=b"", seed=0):
    """a well-formed simple entry: n_points spread over n_contours, mixed flag classes, `instructions` in front of the arrays"""
    ends = [(k + 1) * n_points // n_contours - 1 for k in range(n_contours)]
    stream = plain(n_points, at=seed)
    xs, ys = coords_for(stream, step=1 + seed)
    _, full = entry(ends, stream, xs, ys, trailing)
    if instructions:
        at = 10 + 2 * n_contours
        full = full[:at] + len(instructions).to_bytes(2, "big") + bytes(instructions) + full[at + 2:]
    return full


def raw_simple(n_contours, body):
    """numberOfContours, a bounding box, and whatever `body` says"""
    return i16(n_contours) + b"\0" * 8 + bytes(body)


def rec(child, flags=None, tail=None, more=None):
    """a component record: flags and child, then `tail` as it stands (arguments, scales — or not).  Without flags: word offsets
    (0, 0, or `tail`).  more: None = MORE_COMPONENTS on every record but the composite's last"""
    if flags is None:
        flags, tail = ARGS_XY | ARGS_WORDS, (i16(0) + i16(0) if tail is None else tail)
    return (child, flags, bytes(tail or b""), more)


def xy(dx, dy, words=True):
    return i16(dx) + i16(dy) if words else bytes([dx & 0xFF, dy & 0xFF])


def comp(records, behind=b"", cut=None, header=None):
    """a composite entry of `records`; behind: bytes behind the last record; cut: keep that many bytes of the body"""
    def build(gid_of):
        body = bytearray()
        for k, (child, flags, tail, more) in enumerate(records):
            if more is None:
                more = k + 1 < len(records)
            flags = (flags | MORE) if more else (flags & ~MORE)
            body += flags.to_bytes(2, "big") + (gid_of(child) if isinstance(child, str) else int(child)).to_bytes(2, "big") + tail
        body += bytes(behind)
        if cut is not None:
            body = body[:cut]
        return (i16(-1) + b"\0" * 8 if header is None else bytes(header)) + bytes(body)
    return build


class Forest:
    def __init__(self):
        self.names, self.defs = [], {}

    def add(self, name, body):
        assert name not in self.defs, name
        self.names.append(name)
        self.defs[name] = body
        return name

    def gid(self, name):
        return self.names.index(name)

    def entries(self):
        index = {n: i for i, n in enumerate(self.names)}
        return [d(index.__getitem__) if callable(d) else bytes(d) for d in (self.defs[n] for n in self.names)]

    def tables(self, loca_long=True, **kw):
        return pack(self.entries(), loca_long, **kw)


def pack(entries, loca_long=True, num_glyphs=None, loca_entries=None, offsets=None, lead=0, glyf_cut=None):
    """entries back to back and unpadded (short loca: each padded to an even length; lead: zero bytes in front, which makes every
    short offset odd when lead is 2 mod 4).  offsets: the loca values to write instead (bytes).  glyf_cut: drop the table's tail"""
    data, offs = bytearray(b"\0" * lead), [lead]
    for e in entries:
        data += e
        if not loca_long:
            data += b"\0" * (len(data) % 2)
        offs.append(len(data))
    if offsets is not None:
        offs = list(offsets)
    if glyf_cut is not None:
        data = data[:glyf_cut]
    if loca_long:
        loca = b"".join(o.to_bytes(4, "big") for o in offs)
    else:
        assert all(o % 2 == 0 and o // 2 <= 0xFFFF for o in offs)
        loca = b"".join((o // 2).to_bytes(2, "big") for o in offs)
    n = len(entries) if num_glyphs is None else num_glyphs
    have = len(offs)
    want = 0xFFFF if n == 0xFFFF else n + 1
    return Tables(loca, bytes(data), n, min(want, have) if loca_entries is None else loca_entries, 1 if loca_long else 0)


def font_of(t, mapped=None):
    """a TrueType font file around the tables (what FontManager.add_font_data loads): the scaffold of glyf_edge_entries.font_with_entries
    with `loca`, `glyf` and the loca format replaced; maxp.numGlyphs is t.num_glyphs.  Glyph id g > 0 has code point 0xFF + g;
    mapped: the glyph ids that keep theirs (None: all)"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    from glyf_edge_entries import font_with_entries
    assert t.num_glyphs >= 1
    f = TTFont(io.BytesIO(font_with_entries([b"\0\0"] * (t.num_glyphs - 1))), recalcBBoxes=False, recalcTimestamp=False)
    glyf, loca = DefaultTable("glyf"), DefaultTable("loca")
    glyf.data, loca.data = t.glyf, t.loca
    f["head"].indexToLocFormat = t.loca_long
    f["glyf"], f["loca"] = glyf, loca
    if mapped is not None:
        for st in f["cmap"].tables:
            st.cmap = {cp: name for cp, name in st.cmap.items() if cp - 0xFF in mapped}
    out = io.BytesIO()
    f.save(out)
    return out.getvalue()


# ---- the cases: name -> function(forest, prefix) that adds its glyphs; the glyph `prefix` is the one the case is about ----

LEAF_A, LEAF_B = simple(4), simple(9, 2, instructions=b"\x40\x01\x02\xb0", seed=3)   # B: instructions between end points and arrays


def _with_leaves(fn):
    def case(f, p):
        if "leafA" not in f.defs:
            f.add("leafA", LEAF_A)
            f.add("leafB", LEAF_B)
        fn(f, p)
    return case


CASES = {}


def _case(name, fn):
    assert name not in CASES, name
    CASES[name] = _with_leaves(fn)


def _single(name, records_fn, **kw):
    _case(name, lambda f, p: f.add(p, comp(records_fn(), **kw)))


# argument forms
_single("args_words", lambda: [rec("leafA", ARGS_XY | ARGS_WORDS, xy(300, -200)), rec("leafB", ARGS_XY | ARGS_WORDS, xy(-32768, 32767))])
_single("args_bytes_negative", lambda: [rec("leafA", ARGS_XY, xy(-5, -128, words=False)), rec("leafB", ARGS_XY, xy(127, -1, words=False))])
# anchor form: the two point numbers are NOT consumed, so the next record is read from where they stand.  Here they spell a record
# of their own (flags 0x0002: byte offsets, no MORE; child: leafB's id follows) — beside the same bytes behind an XY record
_case("args_anchor_bytes_not_consumed", lambda f, p: f.add(p, comp([rec("leafA", 0, b"\x00\x02", more=True), rec("leafB", ARGS_XY, xy(7, 9, False))])))
_case("args_xy_bytes_consumed_neighbour", lambda f, p: f.add(p, comp([rec("leafA", ARGS_XY, b"\x00\x02", more=True), rec("leafB", ARGS_XY, xy(7, 9, False))])))
# anchor words with a scale behind: the scale is read from the first argument word
_single("args_anchor_words_with_scale", lambda: [rec("leafA", ARGS_WORDS | SCALE, i16(0x2000) + i16(0x1234) + f2(0.5), more=False)])
_single("args_xy_words_with_scale_neighbour", lambda: [rec("leafA", ARGS_XY | ARGS_WORDS | SCALE, i16(0x2000) + i16(0x1234) + f2(0.5))])

# scale forms and their precedence
_T22 = f2(0.75) + f2(-0.3333) + f2(0.1234) + f2(1.5)
_single("scale_uniform", lambda: [rec("leafA", ARGS_XY | SCALE, xy(1, 2, False) + f2(0.3333))])
_single("scale_xy", lambda: [rec("leafA", ARGS_XY | XY_SCALE, xy(1, 2, False) + f2(0.3333) + f2(-1.25))])
_single("scale_two_by_two", lambda: [rec("leafA", ARGS_XY | TWO_BY_TWO, xy(1, 2, False) + _T22)])
_single("scale_two_by_two_over_xy", lambda: [rec("leafA", ARGS_XY | TWO_BY_TWO | XY_SCALE, xy(1, 2, False) + _T22), rec("leafB")])
_single("scale_xy_over_uniform", lambda: [rec("leafA", ARGS_XY | XY_SCALE | SCALE, xy(1, 2, False) + f2(0.3333) + f2(-1.25)), rec("leafB", tail=xy(1, 1))])
_single("scale_two_by_two_over_uniform", lambda: [rec("leafA", ARGS_XY | TWO_BY_TWO | SCALE, xy(1, 2, False) + _T22), rec("leafB", tail=xy(1, 1))])
_single("scale_all_three_bits", lambda: [rec("leafA", ARGS_XY | TWO_BY_TWO | XY_SCALE | SCALE, xy(1, 2, False) + _T22), rec("leafB", tail=xy(1, 1))])
# F2Dot14 extremes and products that round in f32
_single("f2dot14_extremes", lambda: [rec("leafA", ARGS_XY | XY_SCALE, xy(0, 0, False) + i16(-32768) + i16(32767)),
                                      rec("leafB", ARGS_XY | TWO_BY_TWO, xy(0, 0, False) + i16(32767) + i16(-32768) + i16(1) + i16(-1))])


def _nested(levels):
    """composites under composites, each with a 2x2 and an offset whose products are not exact in f32"""
    def case(f, p):
        mats = [(0x2AAB, 0x7FFF, -0x5555, 0x1235), (0x7FFF, -0x0001, 0x3333, -0x7FFF), (-0x6789, 0x2AAB, 0x7FFD, 0x5555)]
        below = "leafB"
        for lv in range(levels - 1, -1, -1):
            m = mats[lv % 3]
            name = p if lv == 0 else f"{p}/{lv}"
            f.add(name, comp([rec("leafA", ARGS_XY | ARGS_WORDS | SCALE, xy(12345 - lv, -7) + i16(0x2AAB + lv)),
                              rec(below, ARGS_XY | ARGS_WORDS | TWO_BY_TWO, xy(-32767 + lv, 12347) + b"".join(i16(v) for v in m))]))
            below = name
    return case


_case("compose_two_levels", _nested(2))
_case("compose_three_levels", _nested(3))


# a record truncated at each `has`, beside the whole record; a leaf in front stays in every case
def _truncated(flags, tail, keep):
    """the second record is cut to `keep` bytes (None: whole)"""
    def records():
        return [rec("leafA", tail=xy(1, 1)), rec("leafB", flags, tail, more=False)]
    first = 4 + 4
    return lambda f, p: f.add(p, comp(records(), cut=None if keep is None else first + keep))


for _name, _flags, _tail in (("words", ARGS_XY | ARGS_WORDS, xy(5, 6)), ("bytes", ARGS_XY, xy(5, 6, False)),
                             ("scale", ARGS_XY | SCALE, xy(5, 6, False) + f2(0.5)), ("xy_scale", ARGS_XY | XY_SCALE, xy(5, 6, False) + f2(0.5) + f2(0.25)),
                             ("two_by_two", ARGS_XY | TWO_BY_TWO, xy(5, 6, False) + _T22)):
    _whole = 4 + len(_tail)
    _case(f"truncated_{_name}_whole", _truncated(_flags, _tail, None))
    _case(f"truncated_{_name}_last_byte_missing", _truncated(_flags, _tail, _whole - 1))
    _case(f"truncated_{_name}_header_only", _truncated(_flags, _tail, 4))
    _case(f"truncated_{_name}_header_three_bytes", _truncated(_flags, _tail, 3))
_case("truncated_bytes_args_one_byte", _truncated(ARGS_XY, xy(5, 6, False), 5))
_case("truncated_scale_args_only", _truncated(ARGS_XY | SCALE, xy(5, 6, False) + f2(0.5), 6))

# children that do not resolve (each is skipped, the leaf behind it is delivered)
_single("child_ffff", lambda: [rec(0xFFFF), rec("leafB")])
_single("child_past_loca", lambda: [rec(0xFFF0), rec("leafB")])
_case("child_empty_range", lambda f, p: (f.add(p + "/empty", b""), f.add(p, comp([rec(p + "/empty"), rec("leafB")]))))
# children that resolve and deliver nothing, or fail
_case("child_no_contours_two_bytes", lambda f, p: (f.add(p + "/c", b"\0\0"), f.add(p, comp([rec(p + "/c"), rec("leafB")]))))
_case("child_no_contours_one_byte_fails", lambda f, p: (f.add(p + "/c", b"\0"), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_no_contours_with_body", lambda f, p: (f.add(p + "/c", raw_simple(0, b"\1\2\3\4")), f.add(p, comp([rec(p + "/c"), rec("leafB")]))))
_case("child_lone_point", lambda f, p: (f.add(p + "/c", raw_simple(1, i16(0) + i16(0) + b"\x01\x05\x05")),
                                         f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_simple_header_nine_bytes", lambda f, p: (f.add(p + "/c", raw_simple(1, b"")[:9]), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_composite_header_nine_bytes", lambda f, p: (f.add(p + "/c", raw_simple(-1, b"")[:9]), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_composite_header_only", lambda f, p: (f.add(p + "/c", raw_simple(-1, b"")), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_last_end_ffff_fails_in_the_middle", lambda f, p: (f.add(p + "/c", raw_simple(2, i16(3) + i16(-1) + i16(0))),
                                                               f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_end_points_past_the_entry", lambda f, p: (f.add(p + "/c", raw_simple(3, i16(3) + i16(5))), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_no_instruction_length", lambda f, p: (f.add(p + "/c", raw_simple(1, i16(3) + b"\0")), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_instructions_past_the_entry", lambda f, p: (f.add(p + "/c", raw_simple(1, i16(3) + i16(9) + b"\0" * 8)), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_instructions_to_the_end", lambda f, p: (f.add(p + "/c", raw_simple(1, i16(3) + i16(8) + b"\0" * 8)), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))


def _stored(total):
    """a simple entry whose stored bytes (end points + what lies behind the instructions) are exactly `total`"""
    base = simple(6)
    return simple(6, trailing=bytes((7 * i + 1) & 0xFF for i in range(total - (len(base) - 12))))


_case("child_entry_of_32k", lambda f, p: (f.add(p + "/c", _stored(MAX_ENTRY)), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_case("child_entry_past_32k", lambda f, p: (f.add(p + "/c", _stored(MAX_ENTRY + 1)), f.add(p, comp([rec("leafA"), rec(p + "/c"), rec("leafB")]))))
_single("no_more_components_with_bytes_behind", lambda: [rec("leafA", more=False), rec("leafB", more=False)], behind=b"\xff" * 5)


def _chain(length):
    """composites p, p/1, .. p/(length - 1), each a leaf and the next; the last names leafB: leafB sits at depth `length`"""
    def case(f, p):
        for k in range(length - 1, -1, -1):
            below = "leafB" if k == length - 1 else f"{p}/{k + 1}"
            f.add(p if k == 0 else f"{p}/{k}", comp([rec("leafA", ARGS_XY, xy(k, -k, False)), rec(below, ARGS_XY | SCALE, xy(1, 0, False) + f2(0.999))]))
    return case


_case("chain_depth_31", _chain(31))
_case("chain_depth_32", _chain(32))
_case("chain_depth_33", _chain(33))
_case("names_itself", lambda f, p: f.add(p, comp([rec("leafA", ARGS_XY, xy(1, 1, False)), rec(p, ARGS_XY | SCALE, xy(3, 0, False) + f2(-0.5)), rec("leafB")])))
_case("cycle_of_two_with_a_leaf_in_front", lambda f, p: (f.add(p, comp([rec("leafB"), rec(p + "/other", ARGS_XY | XY_SCALE, xy(0, 9, False) + f2(1.1) + f2(0.9))])),
                                                           f.add(p + "/other", comp([rec(p, ARGS_XY, xy(2, 2, False)), rec("leafA")]))))


def _fan(f, name, child, n, flags=ARGS_XY, tail_of=lambda i: xy(i % 100, i // 100, False)):
    f.add(name, comp([rec(child, flags, tail_of(i)) for i in range(n)]))


_case("glyph_of_600_leaves", lambda f, p: (_fan(f, p + "/row", "leafA", 25), _fan(f, p, p + "/row", 24)))

LONG_CASES = sorted(CASES)


def forest_of(names, order=1):
    """the named cases side by side in one font; order: -1 adds them in reverse"""
    f = Forest()
    for name in list(names)[::order]:
        CASES[name](f, name)
    return f


def case_tables(name):
    return forest_of([name]).tables()


# ---- fonts that are about `loca` itself, and fonts at the bounds: name -> Tables ----

def _loca_fonts():
    out = {}
    f = forest_of(["args_words", "compose_three_levels", "child_lone_point", "glyph_of_600_leaves"])
    out["short_loca"] = f.tables(loca_long=False)
    out["short_loca_odd_offsets"] = f.tables(loca_long=False, lead=2)
    e = f.entries()
    long = pack(e)
    offs = [int.from_bytes(long.loca[4 * i:4 * i + 4], "big") for i in range(len(e) + 1)]
    top = f.gid("args_words")
    # two glyph ids share one range: the last glyph id's range is leafA's (the glyph id in front of it runs backwards)
    out["two_glyph_ids_share_a_range"] = pack(e + [b"", b""], offsets=offs + [offs[f.gid("leafA")], offs[f.gid("leafA") + 1]])
    # the last glyph id's range ends past glyf: it does not resolve, nor does a child naming it
    g = Forest()
    g.add("leafA", LEAF_A), g.add("leafB", LEAF_B)
    g.add("top", comp([rec("leafA"), rec("cut"), rec("leafB")]))
    g.add("cut", LEAF_A)
    out["range_past_glyf"] = g.tables(glyf_cut=len(b"".join(g.entries())) - 1)
    out["range_whole_neighbour"] = g.tables()
    # a range that runs backwards
    ge = g.entries()
    go = [0]
    for x in ge:
        go.append(go[-1] + len(x))
    out["range_backwards"] = pack(ge, offsets=go[:3] + [go[4], go[3]])
    # loca shorter than num_glyphs + 1: the glyph ids behind it do not resolve
    out["loca_shorter_than_num_glyphs"] = pack(e, num_glyphs=len(e) + 5)
    out["loca_cut_in_the_middle"] = Tables(long.loca[:4 * (top + 1)], long.glyf, long.num_glyphs, top + 1, 1)
    out["loca_of_one_entry"] = Tables(long.loca[:4], long.glyf, long.num_glyphs, 1, 1)
    out["no_loca"] = Tables(b"", long.glyf, long.num_glyphs, 0, 1)
    out["no_glyf"] = Tables(long.loca, b"", long.num_glyphs, long.loca_entries, 1)
    return out


LOCA_FONTS = _loca_fonts()


def budget_font(extra):
    """a glyph id that reads exactly MAX_COMPONENTS + extra component records, from a few records by nesting: level k holds four
    records of level k - 1, level 0 four records that resolve to nothing; the top adds what is missing.  No leaf below it"""
    f = Forest()
    f.add("leafA", LEAF_A)
    f.add("n0", comp([rec(0xFFFF, 0)] * 4))
    cost = [1 + 4]                                   # of a record that names level k: itself and what the level reads
    while 1 + 4 * cost[-1] <= MAX_COMPONENTS // 3:
        k = len(cost)
        f.add(f"n{k}", comp([rec(f"n{k - 1}", 0)] * 4))
        cost.append(1 + 4 * cost[-1])
    left, records = MAX_COMPONENTS + extra - 1, []   # (the last record names the leaf)
    for k in range(len(cost) - 1, -1, -1):
        records += [rec(f"n{k}", 0)] * (left // cost[k])
        left %= cost[k]
    records += [rec(0xFFFF, 0)] * left
    f.add("top", comp(records + [rec("leafA")]))
    return f.tables()


def leaves_font(extra):
    """a face of exactly MAX_LEAVES + extra leaves, from a few records by nesting: level k holds 16 records of level k - 1 (level 0
    is a leaf of four points), seven glyph ids hold 8 records of level 4 (2^19 leaves and 559 240 records each: below the
    component budget), and the last glyph id holds what is missing, most significant level first.  Every record shifts by small
    whole numbers"""
    f = Forest()
    f.add("n0", LEAF_A)
    for k in range(1, 5):
        _fan(f, f"n{k}", f"n{k - 1}", 16, tail_of=lambda i: xy(i % 4, i // 4, False))
    for j in range(7):
        _fan(f, f"top{j}", "n4", 8, tail_of=lambda i, j=j: xy(16 * i, j, False))
    left = MAX_LEAVES + extra - sum(16 ** k for k in range(5)) - 7 * 8 * 16 ** 4
    records = []
    for k in range(4, -1, -1):
        records += [rec(f"n{k}", ARGS_XY, xy(len(records) + i, 100, False)) for i in range(left // 16 ** k)]
        left %= 16 ** k
    f.add("last", comp(records))
    return f.tables()


def slots_font(n_leaves):
    """a glyph id of n_leaves leaves of 65537 command slots each (an entry that claims 65535 points and carries none):
    1023 of them stay below 2^26 slots, 1024 pass it"""
    f = Forest()
    f.add("big", raw_simple(1, i16(-2) + i16(0)))
    _fan(f, "row", "big", 32)
    f.add("top", comp([rec("row", 0)] * (n_leaves // 32) + [rec("big", 0)] * (n_leaves % 32)))
    return f.tables()


def count_font(n, deep_at=None, kind="mixed"):
    """a face of n glyph ids.  mixed: leaves, small composites, empty ranges; deep_at: that glyph id heads a chain whose leaf sits
    at depth 31 (its links are the glyph ids around it).  simple: no composite.  composite: no simple glyph (no leaf, no byte)"""
    f = Forest()
    names = [f"g{i}" for i in range(n)]
    links = []
    if deep_at is not None:
        links = [i for i in range(n) if i != deep_at][:31]
        assert len(links) == 31
    chain = [deep_at] + links[:30] if deep_at is not None else []   # composites; links[30] is the leaf at depth 31... of 31 glyph ids
    for i in range(n):
        if deep_at is not None and i in chain:
            k = chain.index(i)
            below = names[chain[k + 1]] if k + 1 < len(chain) else names[links[30]]
            body = comp([rec(names[links[30]], ARGS_XY, xy(k, 1, False)), rec(below, ARGS_XY | SCALE, xy(0, k, False) + f2(0.97))])
        elif deep_at is not None and i == links[30]:
            body = simple(5 + i % 7, seed=i)
        elif kind == "simple":
            body = simple(2 + i % 9, 1 + i % 2, instructions=bytes(i % 4), seed=i)
        elif kind == "composite":
            body = comp([rec(names[(i + 1) % n], ARGS_XY, xy(i % 50, 0, False)), rec(0xFFFF)]) if i % 3 else comp([])
        elif i % 5 == 4:
            body = b""
        elif i % 5 == 3 and i >= 3:
            body = comp([rec(names[i - 3], ARGS_XY, xy(i % 100, -3, False)), rec(names[i - 2], ARGS_XY | XY_SCALE, xy(0, 0, False) + f2(0.5) + f2(1.25))])
        else:
            body = simple(2 + i % 9, 1 + i % 2, instructions=bytes(i % 3), seed=i)
        f.add(names[i], body)
    return f.tables()
