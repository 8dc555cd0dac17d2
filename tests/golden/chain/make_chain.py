"""Regenerate the chain fixture from the REFERENCE libyara (build container only).

    make -f oracle/ref.mk REF=$YARA_REFERENCE -j8   # stock libyara + refdump + yarac
    python tests/golden/chain/make_chain.py

As tests/golden/hexwide: rules and buffer are this project's own; tables.npz and
case.npz hold what stock libyara compiles and finds (verify calls, match lists).
tables.npz also holds the strings' chain links (str_chained_to, str_gap_min,
str_gap_max).  chains_<n>.yarc.gz are stock yarac's output for n two-part chains
of the template chain_rules() (tests/test_gpu_chain_matches.py plants them).
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
sys.path[:0] = [os.path.dirname(os.path.dirname(GOLDEN)), GOLDEN]

import oracle  # noqa: E402
from oracle.tables import read_tables  # noqa: E402
import make_golden  # noqa: E402

SIZE = 48 << 10
SEED = 37
# the rule's strings in order; a chain is one name for all its parts
NAMES = ["two", "three", "open", "wild", "dirty", "vary", "regexp", "text"]
DIRTY = ["dirty"]
CHAIN_COUNTS = [1, 64, 65]
h = bytes.fromhex
H2, T2 = h("10111213"), h("14151617")
H3, M3, T3 = h("20212223"), h("24252627"), h("28292a2b")
HO, TO = h("30313233"), h("34353637")


def z(n):
    return bytes(n)


# (offset, bytes, what it is there for); negative offsets count from the end
PLANTS = [
    (1024, H2 + z(299) + T2, "two: gap min - 1, no match; the head is pruned by the next tail"),
    (2048, H2 + z(300) + T2, "two: gap min"),
    (3072, H2 + z(400) + T2, "two: gap max"),
    (4096, H2 + z(401) + T2, "two: gap max + 1, no match"),
    (5120, H2 + z(16) + H2 + z(320) + T2, "two: one tail confirms two heads"),
    (6144, H2 + z(310) + T2 + z(60) + T2, "two: two tails in range, the second finds the head gone"),
    (7168, H2 + H2 + z(300) + T2, "two: two heads side by side in one tail's reach"),
    (8192, H2, "two: a head without a tail, pruned (scan.c:476) before the next plant's tail"),
    (9216, H2 + z(350) + T2, "two: in range, after a pruned head"),
    (12288, H3 + z(320) + M3 + z(330) + T3, "three: the middle present"),
    (13312, H3 + z(654) + T3, "three: the middle absent"),
    (14336, H3 + z(250) + M3 + z(340) + T3, "three: the middle out of the head's range"),
    (15360, H3 + z(320) + M3 + z(20) + M3 + z(310) + T3, "three: two middles, both chained"),
    (16384, HO + z(299) + TO, "open: gap min - 1"),
    (17408, HO + z(300) + TO, "open: gap min; the tail confirms the head before it too"),
    (18432, TO, "open: a tail with nothing left to confirm"),
    (19456, HO + z(700) + TO, "open: far apart"),
    (20480, h("4f99") + h("40414243") + z(350) + h("45464748"), "wild: offset - 2, length from there"),
    (21504, h("0099") + h("40414243") + z(350) + h("45464748"), "wild: the wildcard's neighbour differs"),
    (22528, h("505000") + h("51525354") + z(350) + h("55565758"), "dirty: two backward results"),
    (23552, h("5000") + h("51525354") + z(350) + h("55565758"), "dirty: one result, the chain dirty"),
    (24576, b"chn42" + z(350) + b"xyz", "regexp: a chain that is never settled"),
    (27648, h("60") + z(9) + h("61626364") + z(6) + h("61626364") + z(320) + h("65666768"),
     "vary: two calls of the head at one offset (B = 10 and 20), the second dropped"),
    (26000, b"chain-literal", "text"),
    (-362, H2 + z(350) + T2, "two: the chain ends at the buffer's last byte"),
]


def chain_rules(n):
    """n two-part chains with atoms of their own: C0 hi lo 01 [300-500] C0 hi lo 02."""
    lines = ["rule chains {", "  strings:"]
    for k in range(n):
        lines.append("    $c%d = { C0 %02X %02X 01 [300-500] C0 %02X %02X 02 }"
                     % (k, k >> 8, k & 255, k >> 8, k & 255))
    return "\n".join(lines + ["  condition:", "    any of them", "}", ""])


def main():
    tmp = os.environ.get("GOLDEN_TMP", "/tmp/yara_amd_golden")
    os.makedirs(tmp, exist_ok=True)
    rules, prefix = os.path.join(HERE, "chain.yar"), os.path.join(tmp, "chain")
    subprocess.run([make_golden.REFDUMP, "tables", rules, prefix + ".tables"], check=True,
                   stdout=subprocess.DEVNULL)
    t = read_tables(prefix + ".tables")
    none = 0xFFFFFFFF
    to = np.array([none if s["chained_to"] is None else s["chained_to"] for s in t.strings], np.uint32)
    np.savez_compressed(
        os.path.join(HERE, "tables.npz"), str_chained_to=to,
        str_gap_min=np.array([s["gap_min"] for s in t.strings], np.uint32).astype(np.int32),
        str_gap_max=np.array([s["gap_max"] for s in t.strings], np.uint32).astype(np.int32),
        **make_golden.tables_dict(t))
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
    # the strings of every name: a chain's parts follow their head
    parts, k = {}, 0
    for name in NAMES:
        parts[name] = [k]
        k += 1
        while k < len(to) and to[k] != none:
            parts[name].append(k)
            k += 1
    assert k == len(t.strings)
    for n in CHAIN_COUNTS:
        src, out = os.path.join(tmp, "chains_%d.yar" % n), os.path.join(tmp, "chains_%d.yarc" % n)
        with open(src, "w") as f:
            f.write(chain_rules(n))
        subprocess.run([make_golden.YARAC, src, out], check=True, stdout=subprocess.DEVNULL)
        with open(out, "rb") as f, open(os.path.join(HERE, "chains_%d.yarc.gz" % n), "wb") as g:
            g.write(gzip.compress(f.read(), 9, mtime=0))
    manifest = dict(generator="tests/golden/chain/make_chain.py", rules="chain.yar",
                    reference="libyara 4.2.1 (stock build, oracle/ref.mk)", size=SIZE, seed=SEED,
                    data_sha=hashlib.sha256(buf.tobytes()).hexdigest(),
                    verify_count=int(len(ver)), match_count=int(len(mt)),
                    strings=parts, dirty=DIRTY, string_count=len(t.strings),
                    chain_counts=CHAIN_COUNTS,
                    plants=[[at, len(b), what] for at, b, what in PLANTS])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
