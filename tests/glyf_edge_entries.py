"""Hand-written `glyf` entries that sit on the edges of the device's decoder (csrc/glyf_decode_kernel.inc): the 64-byte
windows of its flag pass, the 64-point windows of its coordinate and contour passes, the 64-contour windows of its
end-point pass, its limits.  A plain helper module: the case lists, a strict sequential decoder that is the yardstick of
tests/test_gpu_glyf_decode_regimes.py, and `roles`, with which every case proves that it sits where it claims to sit
(tests/test_glyf_edge_entries_host.py).

Window w of the decoder's flag pass covers the part bytes [2 nc + 64 w, 2 nc + 64 w + 64): byte j has lane (j - 2 nc) mod 64.
"""
import io
from collections import namedtuple

import numpy as np

from test_glyf_parts_host import _decode_part

# what the decoder's constants are (csrc/input_form_kernels.hip); tests compare them with the library's own (vgsdf_glyf_limits)
MAX_POINTS, MAX_BYTES, EXPAND_FONT_CACHE = 6144, 30 * 1024, 128

ACCEPTED, MALFORMED, DEVICE_LIMIT = "accepted", "malformed", "device_limit"

ON, XS, YS, REP, XSAME, YSAME = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20


def _u16(b, at):
    return (b[at] << 8) | b[at + 1]


def entry(ends, flag_stream, xs, ys, trailing=b""):
    """-> (the part's bytes as vgsdf.h defines them: end points, flags, x, y [, bytes behind them];
           the `glyf` entry of a font: numberOfContours, bbox, end points, instructionLength 0, the arrays)"""
    e = b"".join(int(v).to_bytes(2, "big") for v in ends)
    arrays = bytes(flag_stream) + bytes(xs) + bytes(ys) + bytes(trailing)
    header = len(ends).to_bytes(2, "big", signed=True) + b"\0" * 8
    return e + arrays, header + e + b"\0\0" + arrays


def font_with_entries(entries):
    """a TrueType font whose glyph i + 1 is the raw entry entries[i] (code point 0x100 + i); glyph 0 is a square"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    from test_gpu_glyf_shapes import _font, _simple
    square = [(100, 100, 1), (600, 100, 1), (600, 600, 1), (100, 600, 1)]
    glyphs = {".notdef": _simple([square])}
    for i in range(len(entries)):
        glyphs[f"e{i}"] = _simple([square])
    scaffold = _font(glyphs, {0x100 + i: f"e{i}" for i in range(len(entries))})
    f = TTFont(io.BytesIO(scaffold), recalcBBoxes=False, recalcTimestamp=False)
    notdef = f["glyf"][".notdef"].compile(f["glyf"])
    notdef += b"\0" * (-len(notdef) % 4)
    data, offs = bytearray(notdef), [0, len(notdef)]
    for e in entries:   # entries lie back to back, unpadded: an entry's length is what the test wrote (long `loca`)
        data += e
        offs.append(len(data))
    glyf, loca = DefaultTable("glyf"), DefaultTable("loca")
    glyf.data = bytes(data) + b"\0" * (-len(data) % 4)
    loca.data = b"".join(o.to_bytes(4, "big") for o in offs)
    f["head"].indexToLocFormat = 1
    f["glyf"], f["loca"] = glyf, loca
    out = io.BytesIO()
    f.save(out)
    return out.getvalue()


# ---- the sequential reading of an entry ----

Layout = namedtuple("Layout", "n_points roles lanes flags x_at y_at y_end why")


def layout(part_bytes, n_contours):
    """One sequential walk over the flag stream, as the specification reads it.  roles[s] / lanes[s] describe byte 2 nc + s of the
    part: "flag", "count", or "behind" (not part of the flags the points need: coordinates, trailing bytes).  flags: the flag
    of every point that the stream covers.  why: None, or the rule of walk_simple (csrc/host/ttf_face.cpp) the entry breaks."""
    b, nc = bytes(part_bytes), int(n_contours)
    n = len(b)
    if nc <= 0 or 2 * nc > n:
        return Layout(0, [], [], [], 0, 0, 0, "end points past the bytes")
    last = _u16(b, 2 * (nc - 1))
    if last == 0xFFFF:
        return Layout(0, ["behind"] * (n - 2 * nc), [s % 64 for s in range(n - 2 * nc)], [], 0, 0, 0, "last end point 0xFFFF")
    n_points = last + 1
    roles, flags, why = [], [], None
    cur, xs, ys = 2 * nc, 0, 0
    while len(flags) < n_points and why is None:
        if cur >= n:
            why = "the stream ends before the points are covered"
            break
        fl = b[cur]
        cur += 1
        roles.append("flag")
        run = 1
        if fl & REP:
            if cur >= n:
                why = "a repeat count behind the entry"
                break
            run += b[cur]
            cur += 1
            roles.append("count")
        if run > n_points - len(flags):
            why = "a run crosses the point count"
            break
        flags += [fl] * run
        xs += run * (1 if fl & XS else (0 if fl & XSAME else 2))
        ys += run * (1 if fl & YS else (0 if fl & YSAME else 2))
    x_at = cur
    roles += ["behind"] * (n - 2 * nc - len(roles))
    lanes = [s % 64 for s in range(n - 2 * nc)]
    if why is None and x_at + xs + ys > n:
        why = "y_end > len"
    return Layout(n_points, roles, lanes, flags, x_at, x_at + xs, x_at + xs + ys, why)


def roles(part_bytes, n_contours):
    """-> [(role, lane)] for the part bytes from 2 * n_contours on"""
    lay = layout(part_bytes, n_contours)
    return list(zip(lay.roles, lay.lanes))


def classify(part_bytes, n_contours, cmd_cap):
    """ACCEPTED, MALFORMED (walk_simple's rules: ttf-parser returns None) or DEVICE_LIMIT (well-formed, beyond the decoder)"""
    lay = layout(part_bytes, n_contours)
    if lay.why is not None:
        return MALFORMED
    if lay.n_points > MAX_POINTS or len(part_bytes) > MAX_BYTES or lay.n_points + 2 * int(n_contours) > int(cmd_cap):
        return DEVICE_LIMIT
    return ACCEPTED


IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def decode_callbacks(part_bytes, n_contours, transform=None):
    """the callbacks of a WELL-FORMED entry (whatever the device's limits say), by tests/test_glyf_parts_host.py's walk"""
    lay = layout(part_bytes, n_contours)
    if lay.why is not None:
        raise ValueError("decode_callbacks: " + lay.why)
    if lay.n_points == 1:
        return []   # a lone point yields nothing
    a, b, c, d, e, f = transform or IDENTITY
    part = {"byte_off": 0, "byte_len": len(part_bytes), "n_contours": int(n_contours), "plain": transform is None,
            "a": a, "b": b, "c": c, "d": d, "e": e, "f": f}
    return _decode_part(part, np.frombuffer(bytes(part_bytes), dtype=np.uint8))


def strict_decode(part_bytes, n_contours, cmd_cap, transform=None):
    """-> the callbacks [(kind, x1, y1, x, y) in f32], or MALFORMED, or DEVICE_LIMIT.  Every refusal is decided by a bound that is
    checked before the byte is read (layout): no exception takes part in it."""
    cls = classify(part_bytes, n_contours, cmd_cap)
    if cls != ACCEPTED:
        return cls
    cmds = decode_callbacks(part_bytes, n_contours, transform)
    assert len(cmds) <= int(cmd_cap)
    return cmds


# ---- building entries ----

def point_flags(stream, n_points):
    """the flags a (well-formed prefix of a) stream gives the first n_points points"""
    out, i = [], 0
    while len(out) < n_points and i < len(stream):
        fl = stream[i]
        i += 1
        run = 1
        if fl & REP and i < len(stream):
            run += stream[i]
            i += 1
        out += [fl] * run
    return out[:n_points]


def coords_for(flags, step=1):
    """x and y arrays that fit the size classes of `flags`, with values that keep moving (no two points alike in a row)"""
    xs, ys = bytearray(), bytearray()
    for i, fl in enumerate(flags):
        if fl & XS:
            xs.append(1 + (i * 7 * step) % 29)
        elif not fl & XSAME:
            xs += int(((i * 37 * step) % 201) - 100).to_bytes(2, "big", signed=True)
        if fl & YS:
            ys.append(1 + (i * 5 * step) % 23)
        elif not fl & YSAME:
            ys += int(((i * 53 * step) % 161) - 80).to_bytes(2, "big", signed=True)
    return bytes(xs), bytes(ys)


def rle(flags):
    """the flag stream font tools write: equal neighbours as one repeat flag + count (runs of at most 256)"""
    out, i = bytearray(), 0
    while i < len(flags):
        run = 1
        while i + run < len(flags) and flags[i + run] == flags[i] and run < 256:
            run += 1
        if run > 1:
            out += bytes([flags[i] | REP, run - 1])
        else:
            out.append(flags[i] & ~REP)
        i += run
    return bytes(out)


# flags without bit 3, of every size class
PLAIN = [0x01, 0x33, 0x15, 0x26, 0x00, 0x37, 0x12, 0x24, 0x07, 0x31, 0x20, 0x16]


def plain(n, at=0):
    return [PLAIN[(at + i) % len(PLAIN)] for i in range(n)]


Case = namedtuple("Case", "name family ends part full n_contours n_points cmd_cap expect check in_font")
# check(case, lay): asserts the case's placement with the sequential layout.  in_font: the host's parts walk lists a part for
# the entry (False where walk_simple's first two rules refuse it before anything is listed: such an entry reaches the device
# through the C ABI only)

CASES = []


def _add(name, family, ends, stream, xs=None, ys=None, trailing=b"", cap_delta=0, expect=ACCEPTED, check=None, in_font=True):
    ends = [int(e) for e in ends]
    n_points = ends[-1] + 1 if ends[-1] != 0xFFFF else 0
    stream = bytes(stream)
    if xs is None:
        xs, ys = coords_for(point_flags(stream, n_points))
    part, full = entry(ends, stream, xs, ys, trailing)
    assert not any(c.name == name for c in CASES), name
    CASES.append(Case(name, family, ends, part, full, len(ends), n_points, n_points + 2 * len(ends) + cap_delta, expect, check, in_font))


def by_family(family, expect=None):
    return [c for c in CASES if c.family == family and (expect is None or c.expect == expect)]


# ---------------------------------------------------------------- A: flag windows

def _a_repeat_at(pos, count, nc):
    # `pos` plain flags, a repeat flag at stream byte `pos`, its count behind it, ten more plain flags
    stream = plain(pos) + [0x35 | REP, count] + plain(10, at=3)
    n = pos + 1 + count + 10
    ends = [n - 1] if nc == 1 else [n // 2, n - 1]

    def check(c, lay):
        assert lay.roles[pos] == "flag" and c.part[2 * nc + pos] & REP and lay.lanes[pos] == pos % 64
        assert lay.roles[pos + 1] == "count" and c.part[2 * nc + pos + 1] == count and lay.lanes[pos + 1] == (pos + 1) % 64
        assert lay.roles[pos + 2] == "flag" and lay.x_at == 2 * nc + pos + 12
    _add(f"A_repeat_lane{pos % 64}_w{pos // 64}_count{count:02x}_nc{nc}", "A", ends, stream, check=check)


for _nc in (1, 2):
    for _count in (0, 1, 8, 0x0F, 0xFF):
        for _pos in (62, 63, 64):
            _a_repeat_at(_pos, _count, _nc)


def _a_count_bit3(pos, counts, name):
    # repeat flags back to back whose counts carry bit 3: flag, count, flag, count, ... from stream byte `pos` on
    stream = plain(pos)
    n = pos
    for k, cnt in enumerate(counts):
        stream += [PLAIN[k % len(PLAIN)] | REP, cnt]
        n += 1 + cnt
    stream += plain(7, at=5)
    n += 7

    def check(c, lay):
        for k, cnt in enumerate(counts):
            assert lay.roles[pos + 2 * k] == "flag" and lay.roles[pos + 2 * k + 1] == "count"
            assert c.part[2 + pos + 2 * k + 1] == cnt and cnt & REP
        assert lay.lanes[pos + 1] == (pos + 1) % 64
    _add(name, "A", [n - 1], stream, check=check)


_a_count_bit3(62, [0x08, 0x0B], "A_count_bit3_on_lane63")
_a_count_bit3(62, [0xFF, 0x88], "A_count_ff_on_lane63")
_a_count_bit3(63, [0x08, 0x0F], "A_count_bit3_on_lane0_after_carry")
_a_count_bit3(63, [0x0F, 0x08, 0x18], "A_count_0f_on_lane0_after_carry")
_a_count_bit3(30, [0x08, 0x0C], "A_count_bit3_in_the_middle")
_a_count_bit3(127, [0x09, 0x1F, 0x08], "A_count_bit3_on_lane0_of_window2")

_COUNTS8 = [0x08, 0x09, 0x0F, 0x18, 0x0C, 0x88, 0x0A]


def _a_alternating(first_window, carry, n_windows, name):
    """n_windows whole windows in which every byte carries bit 3: flag | 8, count | 8, ... — starting with a flag on lane 0
    (carry_count enters as 0) or with the count of a repeat flag on lane 63 of the window in front (it enters as 1)"""
    stream, n = [], 0
    lead = 64 * first_window - (1 if carry else 0)
    stream += plain(lead)
    n += lead
    pairs = 32 * n_windows + (1 if carry else 0)
    for k in range(pairs):
        cnt = _COUNTS8[k % len(_COUNTS8)]
        if carry and k == pairs - 1:
            cnt = 0x03   # (its count is the first byte of the window behind: no bit 3, the all-ones windows end here)
        stream += [PLAIN[k % len(PLAIN)] | REP, cnt]
        n += 1 + cnt
    stream += plain(5, at=2)
    n += 5

    def check(c, lay):
        for w in range(first_window, first_window + n_windows):
            assert all(c.part[2 + s] & REP for s in range(64 * w, 64 * w + 64)), w          # no lane sees a clear bit below it
            assert lay.roles[64 * w] == ("count" if carry else "flag") and lay.lanes[64 * w] == 0
            assert lay.roles[64 * w + 63] == ("flag" if carry else "count")
            assert all(lay.roles[s] != lay.roles[s + 1] for s in range(64 * w, 64 * w + 63))
        assert lay.x_at > 2 + 64 * (first_window + n_windows)
    _add(name, "A", [n - 1], stream, check=check)


_a_alternating(0, False, 2, "A_alternating_carry0_two_windows")
_a_alternating(0, False, 3, "A_alternating_carry0_three_windows")
_a_alternating(1, False, 2, "A_alternating_carry0_from_window1")
_a_alternating(1, True, 2, "A_alternating_carry1_two_windows")
_a_alternating(1, True, 3, "A_alternating_carry1_three_windows")


def _a_flags_end(n_bytes, tail_pair, name):
    # the needed flags end at stream byte n_bytes - 1
    if tail_pair:
        stream = plain(n_bytes - 2) + [0x21 | REP, 4]
        n = n_bytes - 2 + 5
    else:
        stream = plain(n_bytes)
        n = n_bytes

    def check(c, lay):
        assert lay.x_at == 2 + n_bytes and lay.roles[n_bytes - 1] == ("count" if tail_pair else "flag") and lay.roles[n_bytes] == "behind"
        assert lay.lanes[n_bytes - 1] == (n_bytes - 1) % 64
    _add(name, "A", [n - 1], stream, check=check)


_a_flags_end(64, False, "A_flags_end_at_window_end")
_a_flags_end(65, False, "A_flags_end_one_byte_into_window1")
_a_flags_end(128, False, "A_flags_end_at_window1_end")
_a_flags_end(129, False, "A_flags_end_one_byte_into_window2")
_a_flags_end(64, True, "A_flags_end_with_count_on_lane63")
_a_flags_end(65, True, "A_flags_end_with_count_on_lane0")


def _a_flags_end_at_len(stream, n, name, expect=ACCEPTED):
    # every coordinate in the "same" form: the arrays are empty, x_at == y_end == len
    def check(c, lay):
        if expect == ACCEPTED:
            assert lay.x_at == lay.y_end == len(c.part) and all(f & XSAME and f & YSAME and not f & (XS | YS) for f in lay.flags)
    _add(name, "A", [n - 1], stream, xs=b"", ys=b"", expect=expect, check=check)


_SAME = [0x31, 0x30, 0x31, 0x31, 0x30]
_a_flags_end_at_len([_SAME[i % 5] for i in range(10)], 10, "A_flags_end_at_len_plain")
_a_flags_end_at_len([_SAME[i % 5] for i in range(8)] + [0x31 | REP, 6], 15, "A_flags_end_at_len_count_is_the_last_byte")
_a_flags_end_at_len([_SAME[i % 5] for i in range(64)], 64, "A_flags_end_at_len_at_window_end")
_a_flags_end_at_len([_SAME[i % 5] for i in range(65)], 65, "A_flags_end_at_len_one_byte_into_window1")
_a_flags_end_at_len([_SAME[i % 5] for i in range(62)] + [0x30 | REP, 9], 72, "A_flags_end_at_len_count_on_lane63")
_a_flags_end_at_len([_SAME[i % 5] for i in range(63)] + [0x30 | REP, 9], 73, "A_flags_end_at_len_count_on_lane0")


def _a_fake_repeats(n_flags, values, name, want):
    """x bytes (one-byte deltas) behind the last needed flag that look like repeat flags"""
    flags = [0x13 if i % 3 else 0x03 for i in range(n_flags)]     # x: one byte (either sign), y: one byte below
    flags = [f | YS for f in flags]
    n = n_flags
    xs = bytes(values[i % len(values)] for i in range(n))
    ys = bytes((values[(i + 1) % len(values)]) for i in range(n))

    def check(c, lay):
        assert lay.x_at == 2 + n_flags
        behind = [s for s in range(n_flags, len(lay.roles))]
        assert all(lay.roles[s] == "behind" for s in behind) and all(c.part[2 + s] & REP for s in behind)
        assert n_flags // 64 == (n_flags - 1) // 64               # they share the window of the last needed flags
        want(c, lay)
    _add(name, "A", [n - 1], flags, xs=xs, ys=ys, check=check)


def _last_byte_is_a_fake_repeat(c, lay):
    assert c.part[-1] & REP and lay.y_end == len(c.part) and len(c.part) - 2 < 64   # (its "count" would lie behind the entry)


def _fake_runs_cross(c, lay):
    s = lay.x_at - 2
    assert c.part[2 + s] & REP and 1 + c.part[2 + s + 1] > lay.n_points                # (a "run" of that length crosses the point count)


def _fake_fill_window(c, lay):
    assert lay.x_at - 2 < 64 and len(c.part) - 2 >= 64 + 20                            # they fill the window and the next one's start


for _v in (0x08, 0x0F, 0xFF, 0x88):
    _a_fake_repeats(9, [_v], f"A_fake_repeat_last_byte_{_v:02x}", _last_byte_is_a_fake_repeat)
_a_fake_repeats(12, [0xFF, 0xFE, 0x0F], "A_fake_runs_cross_the_point_count", _fake_runs_cross)
_a_fake_repeats(20, [0xFF], "A_fake_runs_of_256_cross_the_point_count", _fake_runs_cross)
_a_fake_repeats(60, [0x08, 0x0F, 0xFF, 0x18, 0x09], "A_fake_repeats_fill_the_window", _fake_fill_window)
_a_fake_repeats(50, [0x08], "A_fake_repeats_08_fill_the_window", _fake_fill_window)
_a_fake_repeats(45, [0xFF, 0x0F], "A_fake_repeats_ff_fill_the_window", _fake_fill_window)


def _a_runs_of_256(k, rest, over, name):
    # k runs of 256 and one of `rest` points; `over`: the last count one larger, so that its run crosses the point count
    stream, n = [], 256 * k + rest
    for i in range(k):
        stream += [(0x11, 0x25, 0x36)[i % 3] | REP, 0xFF]
    stream += [0x07 | REP, rest - 1 + (1 if over else 0)]
    flags = point_flags(stream, n)
    xs, ys = coords_for(flags)
    if over:
        xs, ys = xs + b"\7", ys + b"\5"   # (the arrays as large as the longer run asks for: only the run is wrong)

    def check(c, lay):
        assert all(c.part[2 + 2 * i + 1] == 0xFF and lay.roles[2 * i] == "flag" for i in range(k))
        if over:
            assert lay.why == "a run crosses the point count"
        else:
            assert lay.why is None and len(lay.flags) == n and lay.x_at == 2 + 2 * k + 2
    _add(name, "A", [n - 1], stream, xs=xs, ys=ys, expect=MALFORMED if over else ACCEPTED, check=check)


_a_runs_of_256(3, 200, False, "A_runs_of_256_end_on_the_last_point")
_a_runs_of_256(3, 200, True, "A_runs_of_256_last_count_one_larger")
_a_runs_of_256(2, 256, False, "A_three_runs_of_256_exactly")
_a_runs_of_256(5, 1, False, "A_five_runs_of_256_and_one_point")


# ---------------------------------------------------------------- B: coordinates

def _b_points(n):
    if n <= 129:
        stream = plain(n)
    else:   # runs of changing length and size class (a plain stream of 6144 flags would not fit the byte limit)
        fl, k = [], 0
        while len(fl) < n:
            fl += [PLAIN[k % len(PLAIN)]] * min(1 + (k * 5) % 9, n - len(fl))
            k += 1
        stream = rle(fl)

    def check(c, lay):
        assert lay.n_points == n == len(lay.flags) and len({f & 0x36 for f in lay.flags}) >= min(n, 6) - 1   # mixed size classes
    _add(f"B_points_{n}", "B", [n - 1], stream, check=check)


for _n in (2, 63, 64, 65, 127, 128, 129, MAX_POINTS):
    _b_points(_n)


def _b_words_at(word_points, axis, odd, name):
    # one-byte deltas everywhere, two-byte deltas at `word_points` (around a 64-point boundary); `odd`: at an odd offset
    n = 140
    short, same = (XS, XSAME) if axis == "x" else (YS, YSAME)
    flags = []
    for i in range(n):
        f = ON if i % 4 else 0
        f |= (XS | YS) | (XSAME if i % 2 else 0) | (YSAME if i % 3 else 0)
        if i in word_points or (odd and i == 1):
            f &= ~(short | same)    # two bytes
        if not odd and i == 1:
            f = (f & ~short) | same  # no bytes: the offsets keep their parity
        flags.append(f)

    def check(c, lay):
        size = [1 if f & short else (0 if f & same else 2) for f in lay.flags]
        for p in word_points:
            assert size[p] == 2 and p % 64 in (0, 63)
            assert all(size[q] == 1 for q in (p - 1, p + 1) if q not in word_points)
    _add(name, "B", [n - 1], flags, check=check)


_b_words_at({63}, "x", False, "B_x_word_on_lane63")
_b_words_at({64}, "x", True, "B_x_word_on_lane0_odd_offset")
_b_words_at({63, 64}, "x", True, "B_x_words_on_both_sides_of_point_64")
_b_words_at({63, 64}, "y", False, "B_y_words_on_both_sides_of_point_64")
_b_words_at({127, 128}, "y", True, "B_y_words_on_both_sides_of_point_128")
_b_words_at({63, 64, 127, 128}, "x", False, "B_x_words_at_two_boundaries")


def _b_wrap(axis, sign, two, name):
    """running sums that leave the i16 range between points 63 and 64 (and, `two`, come back between 127 and 128)"""
    n = 150
    dx = [0] * n
    dx[0] = sign * 7
    for i in range(1, 64):
        dx[i] = sign * 520                     # 7 + 63 * 520 = 32767
    dx[64] = sign * 1                          # -> wraps to the other end of the range
    if sign < 0:
        dx[0] = -8                             # -8 - 63 * 520 = -32768
    if two:
        dx[128] = -sign * 1                    # and back
    other = [((i * 13) % 41) - 20 for i in range(n)]
    flags = [ON if i % 5 else 0 for i in range(n)]      # two-byte deltas in both arrays
    a = b"".join(int(v).to_bytes(2, "big", signed=True) for v in dx)
    o = b"".join(int(v).to_bytes(2, "big", signed=True) for v in other)

    def check(c, lay):
        raw = np.cumsum(dx)
        assert -32768 <= raw[63] <= 32767 and abs(int(raw[63])) in (32767, 32768) and not -32768 <= raw[64] <= 32767
        if two:
            assert not -32768 <= raw[127] <= 32767 and -32768 <= raw[128] <= 32767
        else:
            assert not -32768 <= raw[n - 1] <= 32767
    _add(name, "B", [n - 1], flags, xs=a if axis == "x" else o, ys=o if axis == "x" else a, check=check)


_b_wrap("x", +1, False, "B_x_sum_wraps_up_at_point_64")
_b_wrap("x", -1, False, "B_x_sum_wraps_down_at_point_64")
_b_wrap("y", +1, False, "B_y_sum_wraps_up_at_point_64")
_b_wrap("x", +1, True, "B_x_sum_wraps_at_64_and_back_at_128")
_b_wrap("y", -1, True, "B_y_sum_wraps_at_64_and_back_at_128")


def _b_negative_short(points, name):
    n = 135
    flags = []
    for i in range(n):
        f = (ON if i % 3 else 0) | XS | YS | XSAME | YSAME          # one-byte deltas, positive
        if i in points:
            f &= ~(XSAME | YSAME)                                     # negative at the chosen lanes
        flags.append(f)

    def check(c, lay):
        for p in points:
            assert lay.flags[p] & (XS | YS) == (XS | YS) and not lay.flags[p] & (XSAME | YSAME)
        assert {p % 64 for p in points} <= {0, 63}
    _add(name, "B", [n - 1], flags, check=check)


_b_negative_short({0, 63}, "B_negative_bytes_on_lane0_and_lane63")
_b_negative_short({64, 127, 128}, "B_negative_bytes_on_lane0_and_lane63_of_later_windows")
_b_negative_short({63, 64}, "B_negative_bytes_on_both_sides_of_point_64")


def _b_classes(fx, fy, name):
    n = 100
    flags = [(ON if i % 4 else 0) | fx(i) | fy(i) for i in range(n)]

    def check(c, lay):
        sx = {1 if f & XS else (0 if f & XSAME else 2) for f in lay.flags[:64]}
        sy = {1 if f & YS else (0 if f & YSAME else 2) for f in lay.flags[:64]}
        assert sx != sy
    _add(name, "B", [n - 1], flags, check=check)


_b_classes(lambda i: XS | XSAME, lambda i: 0, "B_x_bytes_y_words")
_b_classes(lambda i: 0, lambda i: YS, "B_x_words_y_negative_bytes")
_b_classes(lambda i: XSAME, lambda i: YS | YSAME, "B_x_same_y_bytes")
_b_classes(lambda i: (XS, 0)[i % 2], lambda i: YSAME, "B_x_bytes_and_words_y_same")


# ---------------------------------------------------------------- C: contours

def _c_entry(name, ends, on_of=None, cap_delta=0, expect=ACCEPTED, check=None, family="C"):
    """a plain flag stream (every size class) for the points the end points ask for; on_of(p): point p lies on the curve"""
    n = ends[-1] + 1
    flags = []
    for i in range(n):
        f = PLAIN[i % len(PLAIN)] & ~ON
        if (on_of(i) if on_of else i % 3 != 1):
            f |= ON
        flags.append(f)
    stream = flags if n <= 200 else rle(flags)
    _add(name, family, ends, stream, cap_delta=cap_delta, expect=expect, check=check)


def _ends_of(lengths):
    return list(np.cumsum(lengths) - 1)


def _c_contours(nc):
    lengths = [1 + (k * 3) % 4 for k in range(nc)]
    lengths[0] = 3

    def check(c, lay):
        assert c.n_contours == nc and lay.n_points == sum(lengths) and max(lengths) <= 4
    _c_entry(f"C_contours_{nc}", _ends_of(lengths), check=check)


for _nc in (1, 63, 64, 65, 128, 129, 1000):
    _c_contours(_nc)


def _ends_check(want):
    def check(c, lay):
        assert c.ends[:len(want)] == want
    return check


_c_entry("C_contour_ends_on_point_63", [63, 75], check=_ends_check([63]))
_c_entry("C_contour_ends_on_point_64", [64, 75], check=_ends_check([64]))
_c_entry("C_contour_ends_on_point_127_and_128", [10, 127, 128, 140], check=_ends_check([10, 127, 128]))
_c_entry("C_one_point_contour_on_lane63_on_curve", [62, 63, 75], on_of=lambda p: p == 63 or p % 3 != 1, check=_ends_check([62, 63]))
_c_entry("C_one_point_contour_on_lane63_off_curve", [62, 63, 75], on_of=lambda p: p != 63 and p % 3 != 1, check=_ends_check([62, 63]))
_c_entry("C_one_point_contour_on_lane0_on_curve", [63, 64, 75], on_of=lambda p: p == 64 or p % 3 != 1, check=_ends_check([63, 64]))
_c_entry("C_one_point_contour_on_lane0_off_curve", [63, 64, 75], on_of=lambda p: p != 64 and p % 3 != 1, check=_ends_check([63, 64]))
_c_entry("C_one_off_curve_point_contours_only", [0, 1, 2], on_of=lambda p: False, check=_ends_check([0, 1, 2]))
_c_entry("C_one_off_curve_point_then_a_contour", [0, 20], on_of=lambda p: p not in (0, 5), check=_ends_check([0]))


def _long_check(c, lay):
    first, last = c.ends[0] + 1, c.ends[1]
    assert last - first + 1 > 128 and first // 64 + 2 < last // 64 + 1 and first % 64 != 0   # two whole windows inside the contour


_c_entry("C_contour_of_200_points_through_two_windows", [4, 204, 215], check=_long_check)
_c_entry("C_contour_of_300_points_from_lane63", [62, 362, 370], on_of=lambda p: p % 2 == 0, check=_long_check)


def _c_off_start(first, n_off, name):
    def check(c, lay):
        assert c.ends[0] + 1 == first and first % 64 == 63 and not lay.flags[first] & ON
        assert bool(lay.flags[first + 1] & ON) == (n_off == 1)
    off = set(range(first, first + n_off))
    _c_entry(name, [first - 1, first + 20], on_of=lambda p: p not in off and p % 4 != 2, check=check)


_c_off_start(63, 1, "C_off_curve_start_on_lane63_second_point_on_lane0")
_c_off_start(63, 2, "C_two_off_curve_points_across_point_64")
_c_off_start(127, 1, "C_off_curve_start_on_lane63_of_window1")
_c_off_start(127, 2, "C_two_off_curve_points_across_point_128")


def _c_two_quads(first, last, name):
    def check(c, lay):
        assert last % 64 == 0 and not lay.flags[first] & ON and not lay.flags[last] & ON and lay.flags[first + 1] & ON
        assert c.ends[1] == last and c.ends[0] + 1 == first
    _c_entry(name, [first - 1, last, last + 9], on_of=lambda p: p not in (first, last, last - 3), check=check)


_c_two_quads(50, 64, "C_finish_emits_two_quads_on_lane0")
_c_two_quads(60, 128, "C_finish_emits_two_quads_on_lane0_of_window2")


def _c_non_ascending_at_64(back, name, cap_delta=0, expect=ACCEPTED):
    ends = [2 * k + 1 for k in range(64)]      # 64 contours of two points: 0 .. 127
    ends.append(ends[63] - back)               # contour 64 does not ascend (its `prev` is contour 63's end: the window in front)
    ends += [ends[63] + 6, ends[63] + 12]      # (the last contour's points run out: it stays open)

    def check(c, lay):
        assert c.ends[64] <= c.ends[63] and len(c.ends) == 67
    _c_entry(name, ends, cap_delta=cap_delta, expect=expect, check=check)


_c_non_ascending_at_64(0, "C_end_point_64_equals_end_point_63")
_c_non_ascending_at_64(40, "C_end_point_64_goes_back_into_window0")


def _c_open_end(ends, name, cap_delta=0, expect=ACCEPTED):
    def check(c, lay):
        lengths = [c.ends[0] + 1] + [max(c.ends[k] - c.ends[k - 1], 1) if c.ends[k] > c.ends[k - 1] else 1 for k in range(1, len(c.ends))]
        laid, opened = 0, False
        for ln in lengths:
            if laid < lay.n_points < laid + ln:
                opened = True      # this contour begins inside the points and ends behind them
            laid += ln
        assert opened and laid > lay.n_points
    _c_entry(name, ends, on_of=lambda p: p % 4 != 3, cap_delta=cap_delta, expect=expect, check=check)


_c_open_end([5, 3, 12], "C_open_end_with_filler_slots", cap_delta=3)
# the smallest cmd_cap the header allows (points + 2 contours): the open contour brings at most one callback per point it has
# and no finish(), every other contour at most its points + 2 — a slot is always left for the close() that ends the ring
_c_open_end([5, 3, 12], "C_open_end_smallest_cmd_cap")
_c_open_end([70, 60, 64], "C_open_end_last_point_on_lane0")
_c_open_end([40, 30, 63], "C_open_end_last_point_on_lane63")
_c_open_end([5, 3, 12], "C_open_end_one_slot_short", cap_delta=-1, expect=DEVICE_LIMIT)


# ---------------------------------------------------------------- D: limits, a pair on either side

def _d_points(n, name, expect):
    fl, k = [], 0
    while len(fl) < n:
        fl += [PLAIN[k % len(PLAIN)] | (XSAME if k % 2 else 0)] * min(2 + (k * 7) % 11, n - len(fl))
        k += 1

    def check(c, lay):
        assert lay.n_points == n and lay.why is None and len(c.part) <= MAX_BYTES
    _add(name, "D", [n // 3, n - 1], rle(fl), expect=expect, check=check)


_d_points(MAX_POINTS, "D_points_6144", ACCEPTED)
_d_points(MAX_POINTS + 1, "D_points_6145", DEVICE_LIMIT)


def _d_bytes(total, name, expect):
    n = 40
    stream = plain(n)
    xs, ys = coords_for(stream)
    used = 2 + len(stream) + len(xs) + len(ys)

    def check(c, lay):
        assert len(c.part) == total and lay.y_end == used and lay.why is None   # the bytes behind y_end are nobody's
    _add(name, "D", [n - 1], stream, xs=xs, ys=ys, trailing=bytes((i * 11 + 8) & 0xFF for i in range(total - used)), expect=expect, check=check)


_d_bytes(MAX_BYTES, "D_bytes_30720", ACCEPTED)
_d_bytes(MAX_BYTES + 4, "D_bytes_30724", DEVICE_LIMIT)


def _d_cap(ends, name, cap_delta, expect):
    def check(c, lay):
        assert c.cmd_cap == lay.n_points + 2 * c.n_contours + cap_delta
    _c_entry(name, ends, cap_delta=cap_delta, expect=expect, check=check, family="D")


_d_cap([9, 19, 29], "D_cmd_cap_exact", 0, ACCEPTED)
_d_cap([9, 19, 29], "D_cmd_cap_one_less", -1, DEVICE_LIMIT)
_d_cap([63], "D_cmd_cap_exact_64_points", 0, ACCEPTED)
_d_cap([63], "D_cmd_cap_one_less_64_points", -1, DEVICE_LIMIT)


def _why(rule, **kw):
    def check(c, lay):
        assert lay.why == rule
        for k, v in kw.items():
            assert getattr(lay, k) == v
    return check


def _fine(c, lay):
    assert lay.why is None


# end points past the bytes (three contours, four bytes) | its neighbour: the six bytes are there
_add("D_end_points_past_the_bytes", "D", [1, 3, 5], b"", xs=b"", ys=b"", expect=MALFORMED, in_font=False,
     check=_why("end points past the bytes"))
CASES[-1] = CASES[-1]._replace(part=CASES[-1].part[:4], full=CASES[-1].full[:14])
_add("D_end_points_inside_the_bytes", "D", [1, 3, 5], [0x31 | REP, 5], xs=b"", ys=b"", check=_fine)
# last end point 0xFFFF | 0xFFFE: 65535 points, well-formed, beyond the decoder
_add("D_last_end_point_ffff", "D", [3, 0xFFFF], [0x31 | REP, 0xFF] * 256, xs=b"", ys=b"", expect=MALFORMED, in_font=False,
     check=_why("last end point 0xFFFF"))
_add("D_last_end_point_fffe", "D", [3, 0xFFFE], [0x31 | REP, 0xFF] * 255 + [0x30 | REP, 0xFE], xs=b"", ys=b"", expect=DEVICE_LIMIT,
     check=_why(None, n_points=0xFFFF))
# a repeat count behind the entry | the count is the entry's last byte
_add("D_repeat_count_behind_the_entry", "D", [11], [_SAME[i % 5] for i in range(8)] + [0x31 | REP], xs=b"", ys=b"", expect=MALFORMED,
     check=_why("a repeat count behind the entry"))
_add("D_repeat_count_is_the_last_byte", "D", [11], [_SAME[i % 5] for i in range(8)] + [0x31 | REP, 3], xs=b"", ys=b"", check=_fine)
_add("D_repeat_count_behind_the_entry_flag_on_lane63", "D", [80], [_SAME[i % 5] for i in range(63)] + [0x31 | REP], xs=b"", ys=b"",
     expect=MALFORMED, check=_why("a repeat count behind the entry"))
_add("D_repeat_count_on_lane0_is_the_last_byte", "D", [80], [_SAME[i % 5] for i in range(63)] + [0x31 | REP, 17], xs=b"", ys=b"", check=_fine)
# a run crossing the point count | ending on the last point
_add("D_run_crosses_the_point_count", "D", [20], plain(10) + [0x35 | REP, 11], expect=MALFORMED, check=_why("a run crosses the point count"))
_add("D_run_ends_on_the_last_point", "D", [20], plain(10) + [0x35 | REP, 10], check=_fine)
_add("D_run_crosses_the_point_count_from_lane63", "D", [80], plain(63) + [0x35 | REP, 18], expect=MALFORMED,
     check=_why("a run crosses the point count"))
_add("D_run_from_lane63_ends_on_the_last_point", "D", [80], plain(63) + [0x35 | REP, 17], check=_fine)
# the stream ends before the points are covered | one flag more
_add("D_stream_ends_before_the_points", "D", [9], [_SAME[i % 5] for i in range(9)], xs=b"", ys=b"", expect=MALFORMED,
     check=_why("the stream ends before the points are covered"))
_add("D_stream_covers_the_points", "D", [9], [_SAME[i % 5] for i in range(10)], xs=b"", ys=b"", check=_fine)
_add("D_stream_ends_at_a_window_end_before_the_points", "D", [64], [_SAME[i % 5] for i in range(64)], xs=b"", ys=b"", expect=MALFORMED,
     check=_why("the stream ends before the points are covered"))
_add("D_stream_covers_the_points_one_byte_into_window1", "D", [64], [_SAME[i % 5] for i in range(65)], xs=b"", ys=b"", check=_fine)


# y_end > len: one coordinate byte missing | all there
def _d_y_end(n, name, missing):
    stream = plain(n)
    xs, ys = coords_for(stream)
    _add(name, "D", [n - 1], stream, xs=xs, ys=ys[:len(ys) - missing], expect=MALFORMED if missing else ACCEPTED,
         check=_why("y_end > len") if missing else _fine)


_d_y_end(30, "D_one_coordinate_byte_missing", 1)
_d_y_end(30, "D_every_coordinate_byte_there", 0)
_d_y_end(129, "D_one_coordinate_byte_missing_129_points", 1)
_d_y_end(129, "D_every_coordinate_byte_there_129_points", 0)

BY_NAME = {c.name: c for c in CASES}

# batches of the GPU tests
SMALL_CAP_BATCH = [c.name for c in CASES if c.expect == ACCEPTED and c.cmd_cap < 64]                 # the launch's LDS at its floor
ONE_LARGE_AMONG_SMALL = ["D_cmd_cap_exact", "A_flags_end_at_len_plain", "D_points_6144", "C_open_end_smallest_cmd_cap",
                         "D_every_coordinate_byte_there"]
# (refused case, its accepted neighbour)
NEIGHBOURS = {
    "A_runs_of_256_last_count_one_larger": "A_runs_of_256_end_on_the_last_point",
    "C_open_end_one_slot_short": "C_open_end_smallest_cmd_cap",
    "D_points_6145": "D_points_6144",
    "D_bytes_30724": "D_bytes_30720",
    "D_cmd_cap_one_less": "D_cmd_cap_exact",
    "D_cmd_cap_one_less_64_points": "D_cmd_cap_exact_64_points",
    "D_end_points_past_the_bytes": "D_end_points_inside_the_bytes",
    "D_last_end_point_ffff": "D_end_points_inside_the_bytes",
    "D_last_end_point_fffe": "D_points_6144",
    "D_repeat_count_behind_the_entry": "D_repeat_count_is_the_last_byte",
    "D_repeat_count_behind_the_entry_flag_on_lane63": "D_repeat_count_on_lane0_is_the_last_byte",
    "D_run_crosses_the_point_count": "D_run_ends_on_the_last_point",
    "D_run_crosses_the_point_count_from_lane63": "D_run_from_lane63_ends_on_the_last_point",
    "D_stream_ends_before_the_points": "D_stream_covers_the_points",
    "D_stream_ends_at_a_window_end_before_the_points": "D_stream_covers_the_points_one_byte_into_window1",
    "D_one_coordinate_byte_missing": "D_every_coordinate_byte_there",
    "D_one_coordinate_byte_missing_129_points": "D_every_coordinate_byte_there_129_points",
}


def family_counts():
    return {f: (len(by_family(f)), len(by_family(f, ACCEPTED)), len(by_family(f, MALFORMED)), len(by_family(f, DEVICE_LIMIT))) for f in "ABCD"}


if __name__ == "__main__":
    for fam, (n, a, m, d) in family_counts().items():
        print(f"family {fam}: {n} cases ({a} accepted, {m} malformed, {d} beyond the device's limits)")
