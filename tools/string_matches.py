"""Which literal strings of a compiled rules file match where in a file.

    python tools/string_matches.py [--hex] RULES.yarc FILE [FILE ...]

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

Several files: the output lines are "path string offset length xor", in the
order of the arguments.  Files of at most BLOCK bytes go through batches --
one scan, one pre-verification and one match stage for all files of an arena
(yr_amd_scan_batch_matches) -- the arenas packed below ARENA bytes, the files
split across several arenas when needed; every such file is one buffer, so
its lines are those of a stock scan of the file.  A larger file takes the
block path above.

--hex: the final hex strings too (YR_AMD_MATCH_HEX: hex strings with wildcards
or jumps that are no chain parts), measured on the GPU as yr_re_fast_exec does;
a call of one can be several matches.  The calls left are then those of
regexps, chain parts and base64 strings (and hex calls whose jumps span more
than 64 positions).  Several files go through batches as without --hex
(yr_amd_scanner_set_batch_match_classes): only the files above BLOCK bytes take
the block path.
"""
import gzip
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BLOCK = 1 << 30      # blocks of 1 GiB ...
OVERLAP = 1 << 16    # ... overlapping: a match near a block's edge is taken from the block
                     # that holds OVERLAP / 2 bytes on either side of its start
ARENA = (1 << 32) - (1 << 20)   # a batch's packed arena stays below 4 GiB


def block_path(sc, data):
    """(matches with absolute offsets, calls left) of one file, block-wise."""
    import yara_amd
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
    return yara_amd.merge_matches(blocks), left


def arenas(sizes):
    """The files of at most BLOCK bytes, in order, grouped into arenas whose
    packed size (16-byte aligned starts) stays below ARENA."""
    groups, used = [], 0
    for k, n in enumerate(sizes):
        if n > BLOCK:
            continue
        need = (n + 15) // 16 * 16
        if not groups or used + need > ARENA:
            groups.append([])
            used = 0
        groups[-1].append(k)
        used += need
    return groups


def main():
    argv = [a for a in sys.argv[1:] if a != "--hex"]
    hex_class = len(argv) != len(sys.argv) - 1
    if len(argv) < 2:
        sys.exit(__doc__)
    import numpy as np
    import yara_amd
    opener = gzip.open if argv[0].endswith(".gz") else open
    with opener(argv[0], "rb") as f:
        tables = yara_amd.Tables.from_yarc(f.read(), device=0)
    sc = yara_amd.Scanner(tables)
    if hex_class:
        sc.set_match_classes(yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX)
        sc.set_batch_match_classes(yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX)
    paths = argv[1:]
    if len(paths) == 1:
        matches, left = block_path(sc, np.fromfile(paths[0], dtype=np.uint8))
        for r in matches:
            print(r["string"], r["offset"], r["length"], r["xor_key"])
        print("%d verify calls left for a host verifier" % left, file=sys.stderr)
        return
    sizes = [os.path.getsize(p) for p in paths]
    per, left = [None] * len(paths), 0
    for group in arenas(sizes):
        try:
            m, mo, rest, _ = sc.batch_string_matches(
                [np.fromfile(paths[k], dtype=np.uint8) for k in group])
        except yara_amd.YaraAmdError as e:
            if e.code != yara_amd.INVALID_ARGUMENT:
                raise
            break   # rules with a root match list take no batches: file by file below
        for j, k in enumerate(group):
            per[k] = m[int(mo[j]):int(mo[j + 1])]
        left += len(rest)
    for k, p in enumerate(paths):
        if per[k] is None:   # larger than BLOCK
            per[k], n = block_path(sc, np.fromfile(p, dtype=np.uint8))
            left += n
        for r in per[k]:
            print(p, r["string"], r["offset"], r["length"], r["xor_key"])
    print("%d verify calls left for a host verifier" % left, file=sys.stderr)


if __name__ == "__main__":
    main()
