"""CPU model of what phase 1 of the span kernel (csrc/sdf_span_kernel.inc) finds in a chunk: how many of its 8 blocks of four
groups hold a record.

A chunk is 256 segments = 32 groups of 8 = 8 blocks of 4 groups; every chunk of a glyph is full except the last one, and a
glyph has few chunks, so a large share of the (wave, tile, chunk) sweeps meets a partial chunk.  Both passes of phase 1 visit
only the blocks that hold a record; this model says how many they skip.  Per workload, from the glyph table committed under
tests/golden/ (bitmap size and segment count per glyph):

  wave tile-chunks    sum over glyphs of ceil(pixels / 64) x ceil(segments / 256): the sweeps of one launch (a chunk the
                      chunk-box test skips is counted as swept, so the figure lies slightly above the counting build's)
  in a last chunk     the share of them that meets the glyph's last chunk
  empty blocks        8 - ceil(ceil(records of the last chunk / 8) / 4), averaged over ALL tile-chunks

    python tools/model_phase1_blocks.py [noto_regular fira noto_all]
"""
import csv
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
WORKLOADS = ("noto_regular", "fira", "noto_all")
WAVE, CHUNK, GRP, BLOCK = 64, 256, 8, 4
BLOCKS = CHUNK // (GRP * BLOCK)


def ceil_div(a, b):
    return -(-a // b)


def glyph_table(workload):
    """[(pixels, segments)] of the glyphs that have a bitmap"""
    with open(ROOT / "tests" / "golden" / f"glyphs_{workload}.csv") as fh:
        return [(int(r["bitmap_size"]), int(r["n_segments"])) for r in csv.DictReader(fh) if int(r["bitmap_size"])]


def real_blocks(records):
    """blocks of four groups that hold a record in a chunk of `records` segments"""
    return ceil_div(ceil_div(records, GRP), BLOCK)


def model(glyphs):
    tile_chunks = last = empty = 0
    by_blocks = [0] * (BLOCKS + 1)   # tile-chunks by the number of real blocks of the chunk they meet
    for px, n in glyphs:
        if n == 0:
            continue                  # (no chunk: the kernel's chunk loop does not run)
        waves, chunks = ceil_div(px, WAVE), ceil_div(n, CHUNK)
        b = real_blocks(n - CHUNK * (chunks - 1))
        tile_chunks += waves * chunks
        last += waves
        empty += waves * (BLOCKS - b)
        by_blocks[b] += waves
        by_blocks[BLOCKS] += waves * (chunks - 1)
    return {"glyphs": len(glyphs), "tile_chunks": tile_chunks, "last_share": last / tile_chunks,
            "empty_blocks": empty / tile_chunks, "by_blocks": by_blocks}


def main():
    for workload in sys.argv[1:] or WORKLOADS:
        m = model(glyph_table(workload))
        print(f"{workload}: {m['glyphs']} glyphs, {m['tile_chunks']} wave tile-chunks, {100 * m['last_share']:.1f} % in a glyph's last "
              f"chunk, {m['empty_blocks']:.2f} empty blocks of four per tile-chunk")
        print("  tile-chunks by real blocks 1..8: " + " ".join(str(v) for v in m["by_blocks"][1:]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
