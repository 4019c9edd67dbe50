"""Soak of the three younger decoders over many seeds of the generator kits (tests/charstring_fuzz_kit.py, tests/gvar_fuzz_kit.py):
per seed one face of 192 (`CFF `, CFF2) or 128 (gvar) glyph ids, the comparison of tests/test_decoder_fuzz_host.py (the host reader
against the kit's interpreter / restatement, bit for bit; CFF2 at three positions, gvar at the face's three with its advance
deltas) and, where a device is there, that of tests/test_gpu_decoder_fuzz.py (the store the device builds against the store of the
host reader's table; CFF2 also under two arrays of other blend factors, gvar also batched and the phantom pass; with --batched the
CFF2 face's five arrays of factors once more in ONE vgsdf_fonts_create_charstrings2, every store against its single call's).
Without a device it runs host-only.  At the first difference it prints the seed, the face, the glyph id and the first differing record, and stops
with exit status 1; nothing is tried again.  Every program was run to its end by the kit's interpreter when its face was made.
  python tools/fuzz_decoders.py --seeds 100..199 [--decoder cff|cff2|gvar] [--host-only] [--batched]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_product  # noqa: E402

import charstring2_edge_programs as K2  # noqa: E402
import charstring_fuzz_kit as F  # noqa: E402
import gvar_fuzz_kit as GF  # noqa: E402
import gvar_instances_kit as G  # noqa: E402


def store(ctx, font):
    r = ctx.font_commands_read(font)
    return r["cmd_off"], r["records"], r["context"], font.device_bytes


def frozen(ctx, font):
    cmd_off, records, context, size = store(ctx, font)
    return cmd_off.tobytes(), records.tobytes(), context.tobytes(), size


def device_difference(ctx, built, table, name):
    """None, or a line naming the glyph id and the first record in which the device-built font departs from the table's store"""
    want = ctx.font_create_commands(table["cmd_off"], table["dat_off"], table["kinds"], table["coords"])
    try:
        a, b = store(ctx, built), store(ctx, want)
        if not np.array_equal(a[0], b[0]):
            g = int(np.flatnonzero(np.diff(a[0].astype(np.int64)) != np.diff(b[0].astype(np.int64)))[0])
            return f"{name}: glyph id {g}: the device delivers {int(a[0][g + 1]) - int(a[0][g])} commands, the host {int(b[0][g + 1]) - int(b[0][g])}"
        ra, rb = (np.frombuffer(v[1].tobytes(), np.uint8).reshape(len(v[1]), -1) for v in (a, b))
        bad = np.flatnonzero((ra != rb).any(axis=1))
        if len(bad):
            i = int(bad[0])
            g = int(np.searchsorted(b[0], i, side="right")) - 1
            return f"{name}: glyph id {g}, command {i - int(b[0][g])}: device record {ra[i].tobytes().hex()}, host {rb[i].tobytes().hex()}"
        if a[2].tobytes() != b[2].tobytes():
            i = int(np.flatnonzero(np.frombuffer(a[2].tobytes(), np.uint8) != np.frombuffer(b[2].tobytes(), np.uint8))[0])
            return f"{name}: context byte {i} differs"
        if a[3] != b[3]:
            return f"{name}: device_bytes {a[3]} against {b[3]}"
        return None
    finally:
        built.free()
        want.free()


def charstring_seed(vg, ctx, seed, cff2, batched=False):
    """-> (glyphs compared on the host, glyphs compared on the device, the first difference or None)"""
    face = F.face(seed, cff2)
    font, n, on_host, on_device = face.font(), len(face.glyphs), 0, 0
    singles, first = [], None          # batched: (factors, the single call's store) of every position sent to the device

    def made(d):
        built = make(d)
        if batched and cff2:
            singles.append((np.asarray(d["factors"], np.float32), frozen(ctx, built)))
        return built
    for coords in (F.POSITIONS2 if cff2 else (None,)):
        desc, host = F.host_views(vg, font, cff2, coords)
        diff = F.first_difference(f"{face.name} at {coords}", desc, host, cff2)
        on_host += n
        if diff:
            return on_host, on_device, diff
        if ctx is None:
            continue
        make = ctx.font_create_charstrings2 if cff2 else ctx.font_create_charstrings
        first = first or desc
        diff = device_difference(ctx, made(desc), host, f"{face.name} at {coords} on the device")
        on_device += n
        if diff:
            return on_host, on_device, diff
        if cff2 and coords is None:
            for shift in (0, 3):
                d = dict(desc, **K2.alt_sets(desc, shift))
                want, _ = K2.expected_commands(d, budget=F.MAX_RUN_TOKENS)
                diff = device_difference(ctx, made(d), want, f"{face.name} with the factors of alt_sets(shift={shift}) on the device")
                on_device += n
                if diff:
                    return on_host, on_device, diff
    if singles:
        fonts, status, _ = ctx.fonts_create_charstrings2(first, [f for f, _ in singles])
        try:
            for p, (built, (_, single)) in enumerate(zip(fonts, singles)):
                if built is None or frozen(ctx, built) != single:
                    return on_host, on_device, f"{face.name}: position {p} of the batched call is not the single call's store (status {list(status)})"
            on_device += n * len(fonts)
        finally:
            for built in fonts:
                if built is not None:
                    built.free()
    return on_host, on_device, None


def gvar_seed(vg, ctx, seed):
    f = GF.face(seed)
    n, on_host, on_device, singles, first = GF.N_GLYPHS, 0, 0, [], None
    for coords in f.positions:
        desc, host, advances = GF.host_views(vg, f, coords)
        first = first or desc
        diff = GF.first_difference(f, coords, host, advances)
        on_host += n
        if diff:
            return on_host, on_device, diff
        if ctx is None:
            continue
        font = ctx.font_create_gvar(desc)
        singles.append(frozen(ctx, font))
        diff = device_difference(ctx, font, host, f"{f.name} at {coords} on the device")
        on_device += n
        if diff:
            return on_host, on_device, diff
        d, state = ctx.gvar_advance_deltas(desc)
        if G.bits(d) != G.bits(advances[0]) or state.tolist() != advances[1].tolist():
            g = next(i for i in range(n) if G.bits(d[i:i + 1]) != G.bits(advances[0][i:i + 1]) or state[i] != advances[1][i])
            return on_host, on_device, f"{f.name} at {coords}: glyph id {g}, advance delta: device {d[g]!r} ({state[g]}), host {advances[0][g]!r} ({advances[1][g]})"
    if ctx is not None:
        fonts, status, _ = ctx.fonts_create_gvar(first, f.positions)
        try:
            for p, (font, single) in enumerate(zip(fonts, singles)):
                if font is None or frozen(ctx, font) != single:
                    return on_host, on_device, f"{f.name}: position {p} ({f.positions[p]}) of the batched call is not the single call's store (status {list(status)})"
            on_device += n * len(fonts)
        finally:
            for font in fonts:
                if font is not None:
                    font.free()
    return on_host, on_device, None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", required=True, help="A..B (inclusive)")
    ap.add_argument("--decoder", choices=("cff", "cff2", "gvar"), action="append")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--batched", action="store_true", help="CFF2: the positions once more in one vgsdf_fonts_create_charstrings2")
    args = ap.parse_args()
    a, b = (int(v) for v in args.seeds.split(".."))
    vg = load_product()
    ctx = None
    if not args.host_only and vg.device_count() >= 1:
        import torch  # noqa: F401  (first, so one HIP runtime serves torch and the library)
        ctx = vg.SdfContext(0)
    print(f"seeds {a}..{b}, {'host and device' if ctx is not None else 'host only'}", flush=True)
    status = 0
    for decoder in args.decoder or ("cff", "cff2", "gvar"):
        t0, on_host, on_device, diff = time.time(), 0, 0, None
        for seed in range(a, b + 1):
            h, d, diff = gvar_seed(vg, ctx, seed) if decoder == "gvar" else charstring_seed(vg, ctx, seed, decoder == "cff2", args.batched)
            on_host, on_device = on_host + h, on_device + d
            if diff:
                print(f"{decoder}: DIFFERENCE at seed {seed}: {diff}", flush=True)
                status = 1
                break
        print(f"{decoder}: seeds {a}..{seed}: {on_host} glyph comparisons on the host, {on_device} on the device, "
              f"{'1 difference' if diff else '0 differences'}, {time.time() - t0:.0f} s", flush=True)
        if status:
            break
    if ctx is not None:
        ctx.close()
    return status


if __name__ == "__main__":
    sys.exit(main())
