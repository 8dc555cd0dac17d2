"""Regenerate the hexmatch fixture from the REFERENCE libyara (build container only).

    make -f oracle/ref.mk REF=$YARA_REFERENCE -j8   # stock libyara + refdump
    python tests/golden/hexmatch/make_hexmatch.py

hexmatch.yar and the planted buffer are this project's own; tables.npz holds
the tables stock libyara compiles from the rules (as tests/golden/tables/*.npz)
and case.npz the buffer with stock libyara's verify calls and match lists (as
tests/golden/cases/*.npz).  The shapes the buffer plants are listed in PLANTS.
"""
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

SIZE = 48 << 10
SEED = 29
# YR_STRING.idx order (the chained string compiles into two)
STRINGS = ["two_back", "shortest", "same_start", "wide", "masked", "both_sides", "chain head",
           "chain tail", "text", "regexp"]


def h(text):
    return bytes.fromhex(text)


# (offset, bytes, what it is there for); negative offsets count from the end
PLANTS = [
    # $two_back at the buffer's start: the backward run is cut by offset < min + ...
    (0, h("c1c2c3c4c5c6c7"), "two_back cut by the buffer's start"),
    # four C1 and four C2 before the atom: one call, four offsets
    (256, h("c1c1c1c1c2c2c2c2c3c4c5c6c7"), "two_back: one call, 4 offsets"),
    (300, h("c100c200c3c4c5c6c7"), "two_back: one offset, both jumps 1"),
    # a shorter and a longer continuation: the forward run keeps the shortest
    (512, h("d1d2d3d4d5d6d5d6d5d6"), "shortest: continuations at 0, 2 and 4"),
    (560, h("d1d2d3d400000000d5d6"), "shortest: only the longest"),
    # two atoms reach back to one E1: two calls with the same (string, offset)
    (768, h("e1e2e3e4e5e2e3e4e5"), "same_start: two calls, one offset"),
    (800, h("e1e1e100e2e3e4e5"), "same_start: one call, 3 offsets"),
    # the wide jump: stock libyara matches, the device's window does not hold it
    (1024, h("f1f2f3f4") + bytes(50) + h("f5f6"), "wide: 50 bytes skipped"),
    (1200, h("f1f2f3f4f5f6"), "wide: nothing skipped"),
    (1300, h("f1f2f3f4") + bytes(80) + h("f5f6") + bytes(10) + h("f5f6"), "wide: two ends"),
    # masks and wildcards
    (1536, h("93a7b1ffb2b3b400b5"), "masked: jump 1"),
    (1600, h("9fa0b100b2b3b40000b5"), "masked: jump 2"),
    (1650, h("93a7b1ffb2b3b4b5b5b5"), "masked: jumps 1 and 2"),
    # jumps on both sides of the atom
    (2048, h("81828384000000850086878889"), "both_sides"),
    (2100, h("8182838485858585858586878889"), "both_sides: several starts"),
    (2160, h("81828384818283848500008586878889"), "both_sides: two heads"),
    # a chained string, a text string and a regexp: they stay what they were
    (3072, h("aabbccdd") + bytes(350) + h("eeff1122"), "chain"),
    (4096, b"hexmatch-literal", "text"),
    (4200, b"hm42xyz", "regexp"),
    # the forward run ends at the buffer's last byte
    (-6, h("d1d2d3d4d5d6"), "shortest ends at the last byte"),
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
    rules = os.path.join(HERE, "hexmatch.yar")
    out = os.path.join(tmp, "hexmatch.tables")
    subprocess.run([make_golden.REFDUMP, "tables", rules, out], check=True,
                   stdout=subprocess.DEVNULL)
    t = read_tables(out)
    np.savez_compressed(os.path.join(HERE, "tables.npz"), **make_golden.tables_dict(t))
    buf = buffer()
    data = os.path.join(tmp, "hexmatch.bin")
    buf.tofile(data)
    prefix = os.path.join(tmp, "hexmatch")
    res = subprocess.run([make_golden.REFDUMP, "scan", rules, data, prefix], check=True,
                         capture_output=True, text=True)
    print(res.stdout.strip(), res.stderr.strip())
    ver = np.fromfile(prefix + ".verify", dtype=[("b", "<u8"), ("p", "<u8"), ("k", "<u4")])
    mt = np.fromfile(prefix + ".matches",
                     dtype=[("s", "<u4"), ("o", "<u8"), ("l", "<u4"), ("x", "<u4")])
    np.savez_compressed(os.path.join(HERE, "case.npz"), data=buf, verify_pos=ver["p"],
                        verify_idx=ver["k"], match_string=mt["s"], match_offset=mt["o"],
                        match_len=mt["l"], match_xor=mt["x"])
    manifest = dict(generator="tests/golden/hexmatch/make_hexmatch.py",
                    reference="libyara 4.2.1 (stock build, oracle/ref.mk)",
                    rules="hexmatch.yar", size=SIZE, seed=SEED,
                    data_sha=hashlib.sha256(buf.tobytes()).hexdigest(),
                    verify_count=int(len(ver)), match_count=int(len(mt)),
                    strings=STRINGS, string_count=len(t.strings),
                    plants=[[at, len(b), what] for at, b, what in PLANTS])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
