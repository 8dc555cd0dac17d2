"""Regenerate the hexwide fixture from the REFERENCE libyara (build container only).

    make -f oracle/ref.mk REF=$YARA_REFERENCE -j8   # stock libyara + refdump
    python tests/golden/hexwide/make_hexwide.py

As tests/golden/hexmatch: rules and buffer are this project's own; tables.npz and
case.npz hold what stock libyara compiles and finds (verify calls, match lists).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(os.path.dirname(GOLDEN)), GOLDEN]

import oracle  # noqa: E402
from oracle.tables import read_tables  # noqa: E402
import make_golden  # noqa: E402

SIZE = 48 << 10
SEED = 31
STRINGS = ["fwd", "fwd_end", "back", "back64", "back70", "two", "order", "order_narrow", "limit",
           "chain head", "chain tail", "text", "regexp"]
h = bytes.fromhex


def before(atom, length, marks):   # zeros, then the atom; marks: the byte read backwards at b
    pre = bytearray(length)
    for b, byte in marks:
        pre[length - 1 - b] = byte
    return bytes(pre) + h(atom)


def after(atom, length, marks):   # the atom, then zeros; marks: bytes at bytes_matched b
    buf = bytearray(h(atom)) + bytearray(length)
    for b, text in marks:
        buf[b:b + len(h(text))] = h(text)
    return bytes(buf)


# (offset, bytes, what it is there for); negative offsets count from the end
PLANTS = [
    (0, before("b1b2b3b4", 40, [(39, 0xB5)]), "back: cut by the buffer's start"),
    (512, after("a1a2a3a4", 2, [(4, "a5a6")]), "fwd: continuation at 0"),
    (640, after("a1a2a3a4", 65, [(67, "a5a6")]), "fwd: continuation at 63"),
    (768, after("a1a2a3a4", 66, [(68, "a5a6")]), "fwd: continuation at 64"),
    (896, after("a1a2a3a4", 102, [(104, "a5a6")]), "fwd: continuation at 100"),
    (1024, after("a1a2a3a4", 103, [(105, "a5a6")]), "fwd: continuation at 101, none"),
    (1280, before("b1b2b3b4", 101, [(j, 0xB5) for j in (0, 30, 70, 100)]),
     "back: one call, four starts over two words"),
    (1536, before("c1c2c3c4", 130, [(j, 0xC5) for j in (63, 64, 100, 128, 129)]),
     "back64: shifts by 64 to 128"),
    (1792, before("d1d2d3d4", 201, [(j, 0xD5) for j in (69, 70, 130, 199, 200)]),
     "back70: shifts by 70 to 199"),
    (2048, before("e1e2e3e4", 203, [(j, 0xE6) for j in (0, 50, 100)] +
            [(j, 0xE5) for j in (60, 130, 201)]), "two: spreads sum past 128"),
    (2560, before("b1b2b3b4", 21, [(20, 0xB5)]) + bytes(30) + h("b1b2b3b4"),
     "back: two calls, one offset"),
    (3072, after("f1f2f3f4", 16, [(5, "f5"), (7, "f5"), (9, "f6f6")]),
     "order: the second jump runs from two positions"),
    (3328, after("71727374", 8, [(5, "75"), (7, "75"), (9, "7676")]),
     "order_narrow: the same inside 64 positions"),
    (3584, after("f1f2f3f4", 140, [(74, "f5"), (137, "f6")]), "order: one position a jump"),
    (4096, h("aabbccdd") + bytes(350) + h("eeff1122"), "chain"),
    (4608, b"hexwide-literal", "text"),
    (4700, b"hw42xyz", "regexp"),
    # twenty jumps of 200 each, then the last byte read at 4050 and at 4095: B = 4051, 4096
    (8192, before("9a9b9c9d", 4200, [(201 * k - 1, 0x90) for k in range(1, 21)] +
            [(4050, 0x90), (4095, 0x90)]), "limit: the set reaches YR_RE_SCAN_LIMIT"),
    (-70, h("a7a8a9aa") + bytes(10) + after("a1a2a3a4", 52, [(54, "a5a6")]),
     "fwd ends at the last byte; fwd_end would end past it"),
]


ORDER_EXCLUDED = 2   # records the forward-order condition leaves in the rest: two plants


def main():
    tmp = os.environ.get("GOLDEN_TMP", "/tmp/yara_amd_golden")
    os.makedirs(tmp, exist_ok=True)
    rules, prefix = os.path.join(HERE, "hexwide.yar"), os.path.join(tmp, "hexwide")
    subprocess.run([make_golden.REFDUMP, "tables", rules, prefix + ".tables"], check=True,
                   stdout=subprocess.DEVNULL)
    t = read_tables(prefix + ".tables")
    np.savez_compressed(os.path.join(HERE, "tables.npz"), **make_golden.tables_dict(t))
    buf = oracle.xorshift(SIZE, SEED).copy()
    for at, b, _ in PLANTS:
        buf[at % SIZE:at % SIZE + len(b)] = np.frombuffer(b, np.uint8)
    buf.tofile(prefix + ".bin")
    subprocess.run([make_golden.REFDUMP, "scan", rules, prefix + ".bin", prefix], check=True)
    ver = np.fromfile(prefix + ".verify", dtype=[("b", "<u8"), ("p", "<u8"), ("k", "<u4")])
    mt = np.fromfile(prefix + ".matches",
                     dtype=[("s", "<u4"), ("o", "<u8"), ("l", "<u4"), ("x", "<u4")])
    np.savez_compressed(os.path.join(HERE, "case.npz"), data=buf, verify_pos=ver["p"],
                        verify_idx=ver["k"], match_string=mt["s"], match_offset=mt["o"],
                        match_len=mt["l"], match_xor=mt["x"])
    manifest = dict(generator="tests/golden/hexwide/make_hexwide.py", rules="hexwide.yar",
                    reference="libyara 4.2.1 (stock build, oracle/ref.mk)", size=SIZE, seed=SEED,
                    data_sha=hashlib.sha256(buf.tobytes()).hexdigest(),
                    verify_count=int(len(ver)), match_count=int(len(mt)),
                    strings=STRINGS, string_count=len(t.strings), order_excluded=ORDER_EXCLUDED,
                    plants=[[at, len(b), what] for at, b, what in PLANTS])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
