"""Regenerate the loops fixture from the REFERENCE libyara (build container only).

    make -f oracle/ref.mk REF=$YARA_REFERENCE -j8   # stock libyara + refdump + yarac
    python tests/golden/loops/make_loops.py

loops.yar and the planted buffer are this project's own; tables.npz holds the tables stock
libyara compiles from the rules, rules.yarc.gz the compiled rules file and case.npz the buffer
with stock libyara's verify calls and match lists (as tests/golden/alternation).  The shapes
the buffer plants are listed in PLANTS; manifest.json names the strings of the class.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
REPO = os.path.dirname(os.path.dirname(GOLDEN))
sys.path[:0] = [REPO, GOLDEN, os.path.join(GOLDEN, "alternation")]

import oracle  # noqa: E402
from oracle.tables import read_tables  # noqa: E402
import make_golden  # noqa: E402
from make_alternation import scan  # noqa: E402

SIZE = 16 << 10
SEED = 47
# YR_STRING.idx order
STRINGS = ["plus", "star", "plus_u", "star_u", "alt", "php", "run", "dot", "line", "line_s", "coll_g",
           "coll_u", "eps", "count", "bound", "any", "nocase", "wide", "big", "animals"]
LOOPS = STRINGS[:12]
LETTERS = b"abcdefghijklmnopqrstuvwz"                      # (no x, no y: coll_g, coll_u)


def letters(n):
    return bytes(LETTERS[i % len(LETTERS)] for i in range(n))


def dot(n, early=None):
    """D0t! and a run that ends with ';' after n bytes in all (early: another ';' there)."""
    b = bytearray(b"D0t!" + b"m" * (n - 5) + b";")
    if early:
        b[early - 1] = ord(";")
    return bytes(b)


# (offset, bytes, what it is there for); negative offsets count from the end.  Every plant of a
# string with a backward run starts behind a newline or a byte outside the run's class.
PLANTS = [
    (0, b"ab.php\n", "php: at byte 0, the backward run cut by the buffer's start"),
    (64, b"\npLg1bbbX sTg2bbbX sTg2X pLu3bbbX sTu4bbbX", "greedy the longest, ungreedy the shortest"),
    (128, b"\nLp5abcabd Lp5cd Lp5abab;d", "alt: a loop over an alternation"),
    (192, b"\n  index.php", "php: several backward results (and coll_g's x.php)"),
    (256, b"\nRn6!" + b"a" * 58 + b"z", "run: forward length 63"),
    (384, b"\nRn6!" + b"a" * 59 + b"z", "run: 64"),
    (512, b"\nRn6!" + b"a" * 60 + b"z", "run: 65"),
    (640, b"\nx.php.php", "coll_g: two calls, one (string, offset): the last one's 9 stands"),
    (704, b"\ny.php.php", "coll_u: the first one's 5 stands"),
    (768, b"\nN1a--\n--b! N2a--\n--b! N1a--b!", "newline against . with and without /s"),
    (896, b"\n" + letters(62) + b".php", "php: a backward set of 62 positions"),
    (1024, b"\n" + letters(63) + b".php", "php: 63 positions, settled"),
    (1152, b"\n" + letters(64) + b".php", "php: 64 positions, in the rest"),
    (1280, b"\naaab q1234z  wwx abZZccd nC7AAb w\0D\0008\0a\0a\0b\0 cathouse", "not in the class"),
    (1408, b"\n" + "".join(chr(65 + i % 26) + chr(48 + i % 10) for i in range(70)).encode() + b"9",
     "big: more than 64 instructions"),
    (2048, dot(4095), "dot: a greedy run of 4095"),
    (6400, dot(4096), "dot: 4096, MATCH at YR_RE_SCAN_LIMIT"),
    (10752, dot(4097, early=100), "dot: the far end is cut by YR_RE_SCAN_LIMIT, 100 stands"),
    (-7, b"pLg1bbb", "plus: the run cut by the buffer's end"),
]


def buffer():
    buf = oracle.xorshift(SIZE, SEED).copy()
    for at, b, _ in PLANTS:
        at = at if at >= 0 else SIZE + at
        buf[at:at + len(b)] = np.frombuffer(b, np.uint8)
    return buf


def main():
    tmp = os.environ.get("GOLDEN_TMP", "/tmp/yara_amd_golden")
    os.makedirs(tmp, exist_ok=True)
    rules = os.path.join(HERE, "loops.yar")
    out = os.path.join(tmp, "loops.tables")
    subprocess.run([make_golden.REFDUMP, "tables", rules, out], check=True, stdout=subprocess.DEVNULL)
    t = read_tables(out)
    assert len(t.strings) == len(STRINGS)
    np.savez_compressed(os.path.join(HERE, "tables.npz"), **make_golden.tables_dict(t))
    yarc = os.path.join(tmp, "loops.yarc")
    subprocess.run([make_golden.YARAC, rules, yarc], check=True)
    with open(yarc, "rb") as f, gzip.GzipFile(os.path.join(HERE, "rules.yarc.gz"), "wb", mtime=0) as g:
        g.write(f.read())
    buf = buffer()
    ver, mt = scan(rules, buf, os.path.join(tmp, "loops"), os.path.join(HERE, "case.npz"))
    manifest = dict(generator="tests/golden/loops/make_loops.py",
                    reference="libyara 4.2.1 (stock build, oracle/ref.mk)",
                    rules="loops.yar", size=SIZE, seed=SEED,
                    data_sha=hashlib.sha256(buf.tobytes()).hexdigest(),
                    verify_count=int(len(ver)), match_count=int(len(mt)),
                    strings=STRINGS, loop_strings=LOOPS, alternation_strings=["animals"],
                    plants=[[at, len(b), what] for at, b, what in PLANTS])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for s, o, n in zip(mt["s"], mt["o"], mt["l"]):
        print(STRINGS[s], int(o), int(n))


if __name__ == "__main__":
    main()
