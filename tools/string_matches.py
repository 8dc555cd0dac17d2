"""Which literal strings of a compiled rules file match where in a file.

    python tools/string_matches.py RULES.yarc FILE

Prints one "string offset length xor" line per match of a final string
(include/yara_amd.h: literal, not a chain part, not base64) -- absolute file
offsets, ordered by string, then offset, as stock libyara's match lists -- and
on stderr the number of verify calls left for a host verifier (regexp, hex,
chain-part and base64 strings).  No libyara involved: the tables come from the
.yarc (yr_amd_tables_load_yarc), the matches from the GPU (yr_amd_match_device).

A file of up to BLOCK bytes is one block, and the lines are those of a stock
scan of the file.  A larger file is scanned block-wise, the blocks overlapping
by OVERLAP bytes; of the overlap a block keeps only the matches that start in
its nearer half, so every match printed was decided with at least OVERLAP / 2
bytes of the file on either side of its start (or the file's own end) -- a
FULL_WORD string next to a block's edge is judged by the file's bytes, not by
the edge.  That equals the one-block result for strings shorter than OVERLAP /
2 bytes; the count of calls left is the blocks' sum, calls in the overlaps
counted twice.
"""
import gzip
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BLOCK = 1 << 30      # blocks of 1 GiB ...
OVERLAP = 1 << 16    # ... overlapping: a match near a block's edge is taken from the block
                     # that holds OVERLAP / 2 bytes on either side of its start


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    import numpy as np
    import yara_amd
    opener = gzip.open if sys.argv[1].endswith(".gz") else open
    with opener(sys.argv[1], "rb") as f:
        tables = yara_amd.Tables.from_yarc(f.read(), device=0)
    data = np.fromfile(sys.argv[2], dtype=np.uint8)
    sc = yara_amd.Scanner(tables)
    blocks, left, base = [], 0, 0
    while True:
        last = base + BLOCK >= data.size
        m, rest = sc.string_matches(data[base:base + BLOCK], data_base=base)
        # the overlap with a neighbour: each block keeps its nearer half
        lo = OVERLAP // 2 if base else 0
        hi = BLOCK if last else BLOCK - OVERLAP // 2
        blocks.append((base, m[(m["offset"] >= lo) & (m["offset"] < hi)]))
        left += len(rest)
        if last:
            break
        base += BLOCK - OVERLAP
    for r in yara_amd.merge_matches(blocks):
        print(r["string"], r["offset"], r["length"], r["xor_key"])
    print("%d verify calls left for a host verifier" % left, file=sys.stderr)


if __name__ == "__main__":
    main()
