"""Regenerate the alternation fixture from the REFERENCE libyara (build container only).

    make -f oracle/ref.mk REF=$YARA_REFERENCE -j8   # stock libyara + refdump + yarac
    python tests/golden/alternation/make_alternation.py

alternation.yar and the planted buffer are this project's own; tables.npz holds the
tables stock libyara compiles from the rules, rules.yarc.gz the compiled rules file and
case.npz the buffer with stock libyara's verify calls and match lists (as
tests/golden/hexmatch).  The shapes the buffer plants are listed in PLANTS.

both.yar holds chains beside alternation strings; both_tables.npz (with the chain links,
as tests/golden/chain) and both_case.npz are its tables and its buffer (BOTH_PLANTS) with
stock libyara's lists.
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
sys.path[:0] = [REPO, GOLDEN]

import oracle  # noqa: E402
from oracle.tables import read_tables  # noqa: E402
import make_golden  # noqa: E402

SIZE = 16 << 10
SEED = 31
# YR_STRING.idx order
STRINGS = ["long_first", "short_first", "before", "three", "nested", "jump_in", "wild", "meet",
           "run63", "run64", "run65", "insns65", "far", "animals", "cls", "ncls", "split_b", "split_a",
           "greedy", "ungreedy", "greedy_s", "plus", "boundary", "nocase", "wide"]


def h(text):
    return bytes.fromhex(text)


def run(first, gap):
    return h(first + "e2e3e4e5") + bytes(gap) + h("e7")


# (offset, bytes, what it is there for); negative offsets count from the end
PLANTS = [
    (0, h("090203a1b2c3d4"), "before: starts at byte 0, the backward run cut by the buffer's start"),
    (128, h("aabbccdd010203020300"), "long_first: stock reports 9, the shortest path is 7"),
    (160, h("aabbccdd0102030000"), "long_first: only the short alternative, 7"),
    (192, h("abbbccdd010203020300"), "short_first: the same bytes, 7"),
    (224, h("abbbccdd0102030000"), "short_first: 7"),
    (256, h("09090203a1b2c3d4"), "before: one record, two backward results"),
    (288, h("ff090203a1b2c3d4"), "before: one result"),
    (320, h("1122334455bb"), "three: 1"),
    (336, h("112233446677bb"), "three: 2"),
    (352, h("111122334488 99aabb".replace(" ", "")), "three: 3"),
    (368, h("1122334488bb"), "three: none"),
    (384, h("21222324314125"), "nested: inner first"),
    (400, h("2122232431424325"), "nested: inner second"),
    (416, h("212223243225"), "nested: outer second"),
    (448, h("5152535461006255"), "jump_in: jump 1"),
    (464, h("515253546100006255"), "jump_in: jump 2"),
    (480, h("515253546355"), "jump_in: the other alternative"),
    (496, h("51525354616200006255"), "jump_in: two ends of the jump, one 55"),
    (512, h("71727374008175"), "wild: ?? 81"),
    (528, h("71727374008375"), "wild: ~82 83"),
    (544, h("717273748f8475"), "wild: 8? 84"),
    (560, h("71727374828375"), "wild: none (82 83)"),
    (576, h("9ab1b2b3b4b1b2b3b4c1"), "meet: two records, one (string, offset)"),
    (640, run("e1", 57), "run63"),
    (768, run("f1", 58), "run64"),
    (896, run("f2", 59), "run65: stays in the rest"),
    (1024, h("d0d1d2d301") + bytes(range(3, 0x3B)), "insns65: 65 instructions, not in the class"),
    (1152, b"dogsdoghouse cathousebirdhouse", "animals"),
    (1216, b"class7c classxc nocls7z noclsxz", "cls, ncls"),
    (1280, b"klmnxy klmny klmnxxy opqrxy opqry", "split_b, split_a"),
    (1344, b"abXcdcd ebXcdcd ibXcdcd", "greedy 7, ungreedy 5, greedy_s 7"),
    (1408, b"ab\ncd eb\ncd ib\ncd abXYZWcd", "newline in the gap: only /s matches; a gap of 4"),
    (1472, b"zqqqc worda BlueFish r\0e\0d\0b\0i\0r\0d\0", "not in the class"),
    (1600, h("7a7b7c7d") + bytes(80) + h("7e7f"), "far: a final hex string the wave-wide path settles"),
    (-9, b"birdhouse", "animals: ends at the last byte"),
]


LONG, TWO_H, TWO_T = h("aabbccdd010203020300"), h("10111213"), h("14151617")
BOTH_SIZE = 8 << 10
BOTH_PLANTS = [
    (0, h("a3a3") + bytes(62) + h("b1b2b3b4"), "edge: the atom at 64, stock: (1, 67)"),
    (160, LONG, "long_first: 9, ahead of every chain"),
    (512, TWO_H + bytes(100) + LONG + bytes(190) + TWO_T, "two: gap 300, long_first inside the gap"),
    (1024, TWO_H + bytes(16) + TWO_H + bytes(320) + TWO_T, "two: one tail confirms two heads"),
    (1536, h("09090203a1b2c3d4") + TWO_H + bytes(401) + TWO_T, "before: two results; two: gap max + 1"),
    (2560, h("4f9940414243") + bytes(150) + h("ff090203a1b2c3d4") + bytes(192) + h("45464748"),
     "wild: offset - 2; before inside its gap"),
    (3584, h("202122233233") + bytes(350) + h("24252627"), "mixed: stock matches, the device leaves it"),
    (4608, TWO_H + bytes(350) + TWO_T + LONG, "two, long_first right behind the tail"),
    (-9, h("aabbccdd0102030203"), "long_first: ends at the last byte"),
]


def buffer(size=SIZE, seed=SEED, plants=PLANTS):
    buf = oracle.xorshift(size, seed).copy()
    for at, b, _ in plants:
        at = at if at >= 0 else size + at
        buf[at:at + len(b)] = np.frombuffer(b, np.uint8)
    return buf


def scan(rules, buf, prefix, out):
    """case.npz: the buffer with stock libyara's verify calls and match lists."""
    buf.tofile(prefix + ".bin")
    res = subprocess.run([make_golden.REFDUMP, "scan", rules, prefix + ".bin", prefix], check=True,
                         capture_output=True, text=True)
    print(res.stdout.strip(), res.stderr.strip())
    ver = np.fromfile(prefix + ".verify", dtype=[("b", "<u8"), ("p", "<u8"), ("k", "<u4")])
    mt = np.fromfile(prefix + ".matches",
                     dtype=[("s", "<u4"), ("o", "<u8"), ("l", "<u4"), ("x", "<u4")])
    np.savez_compressed(out, data=buf, verify_pos=ver["p"], verify_idx=ver["k"], match_string=mt["s"],
                        match_offset=mt["o"], match_len=mt["l"], match_xor=mt["x"])
    return ver, mt


def both(tmp):
    rules, prefix = os.path.join(HERE, "both.yar"), os.path.join(tmp, "both")
    subprocess.run([make_golden.REFDUMP, "tables", rules, prefix + ".tables"], check=True,
                   stdout=subprocess.DEVNULL)
    t = read_tables(prefix + ".tables")
    to = [0xFFFFFFFF if s["chained_to"] is None else s["chained_to"] for s in t.strings]
    np.savez_compressed(
        os.path.join(HERE, "both_tables.npz"), str_chained_to=np.array(to, np.uint32),
        str_gap_min=np.array([s["gap_min"] for s in t.strings], np.uint32).astype(np.int32),
        str_gap_max=np.array([s["gap_max"] for s in t.strings], np.uint32).astype(np.int32),
        **make_golden.tables_dict(t))
    _, mt = scan(rules, buffer(BOTH_SIZE, SEED + 1, BOTH_PLANTS), prefix,
                 os.path.join(HERE, "both_case.npz"))
    for s, o, n in zip(mt["s"], mt["o"], mt["l"]):
        print("both: string", int(s), int(o), int(n))


def main():
    tmp = os.environ.get("GOLDEN_TMP", "/tmp/yara_amd_golden")
    os.makedirs(tmp, exist_ok=True)
    both(tmp)
    if sys.argv[1:] == ["both"]:
        return
    rules = os.path.join(HERE, "alternation.yar")
    out = os.path.join(tmp, "alternation.tables")
    subprocess.run([make_golden.REFDUMP, "tables", rules, out], check=True,
                   stdout=subprocess.DEVNULL)
    t = read_tables(out)
    np.savez_compressed(os.path.join(HERE, "tables.npz"), **make_golden.tables_dict(t))
    yarc = os.path.join(tmp, "alternation.yarc")
    subprocess.run([make_golden.YARAC, rules, yarc], check=True)
    with open(yarc, "rb") as f, gzip.GzipFile(os.path.join(HERE, "rules.yarc.gz"), "wb", mtime=0) as g:
        g.write(f.read())
    buf = buffer()
    ver, mt = scan(rules, buf, os.path.join(tmp, "alternation"), os.path.join(HERE, "case.npz"))
    manifest = dict(generator="tests/golden/alternation/make_alternation.py",
                    reference="libyara 4.2.1 (stock build, oracle/ref.mk)",
                    rules="alternation.yar", size=SIZE, seed=SEED,
                    data_sha=hashlib.sha256(buf.tobytes()).hexdigest(),
                    verify_count=int(len(ver)), match_count=int(len(mt)),
                    strings=STRINGS, string_count=len(t.strings),
                    plants=[[at, len(b), what] for at, b, what in PLANTS])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for s, o, n in zip(mt["s"], mt["o"], mt["l"]):
        print(STRINGS[s], int(o), int(n))


if __name__ == "__main__":
    main()
