"""Record the long-match-list fixtures from the REFERENCE libyara (build container only).

    make -f oracle/ref.mk REF=<reference tree> -j8   # stock libyara + refdump
    python tests/golden/make_lists.py

For rules/lists31.yar and rules/lists70.yar (match lists of up to 31 and up to
70 entries: pre-verification's keep mask at its width and past it) the stock
compiler's tables go to ``tables/<set>.npz``, and a stock scan of
``planted_lists.lists_buffer`` with the verify-call probe (oracle/refhook.c) to
``cases/<set>_64K.npz`` (the verify-call stream and the match set, the arrays
of make_golden.py's cases); ``lists.json`` holds sizes, seeds, counts and
digests.  Nothing else is written: golden.json and every other fixture stay as
they are (tests/test_long_lists.py reads these files only).
"""
import json
import os
import subprocess

import numpy as np

import make_golden as mg
import planted_lists as planted
from make_golden import HERE, REFDUMP, TMP, oracle, read_tables

SIZE = (64 << 10) + 77
SETS = {"lists31": 31, "lists70": 70}   # set -> seed of its buffer
MAX_FIXTURE = 483175                    # the largest file under cases/ before these


def main():
    os.makedirs(TMP, exist_ok=True)
    out = dict(generator="tests/golden/make_lists.py",
               reference="libyara 4.2.1 (stock build, oracle/ref.mk)", cases={})
    for name, seed in SETS.items():
        rules = os.path.join(HERE, "rules", "%s.yar" % name)
        dump = os.path.join(TMP, "%s.tables" % name)
        subprocess.run([REFDUMP, "tables", rules, dump], check=True, stdout=subprocess.DEVNULL)
        t = read_tables(dump)
        tables = os.path.join(HERE, "tables", "%s.npz" % name)
        np.savez_compressed(tables, **mg.tables_dict(t))

        buf = planted.lists_buffer(oracle.xorshift, name, SIZE, seed)
        data = os.path.join(TMP, "data_%s.bin" % name)
        buf.tofile(data)
        prefix = os.path.join(TMP, "%s_64K" % name)
        res = subprocess.run([REFDUMP, "scan", rules, data, prefix], check=False,
                             capture_output=True, text=True)
        print(name, res.stdout.strip(), res.stderr.strip())
        rc = int(res.stdout.split("rc=")[1].split()[0])
        ver = np.fromfile(prefix + ".verify", dtype=[("b", "<u8"), ("p", "<u8"), ("k", "<u4")])
        mt = np.fromfile(prefix + ".matches",
                         dtype=[("s", "<u4"), ("o", "<u8"), ("l", "<u4"), ("x", "<u4")])
        hit = np.fromfile(prefix + ".rules", dtype=np.uint8)
        case = os.path.join(HERE, "cases", "%s_64K.npz" % name)
        np.savez_compressed(case, verify_base=ver["b"], verify_pos=ver["p"], verify_idx=ver["k"],
                            match_string=mt["s"], match_offset=mt["o"], match_len=mt["l"],
                            match_xor=mt["x"], rules_matching=hit)
        for f in (tables, case):
            assert os.path.getsize(f) <= MAX_FIXTURE, (f, os.path.getsize(f))
        out["cases"]["%s_64K" % name] = dict(
            rules=name, data=["lists", name, seed, SIZE], size=SIZE, rc=rc,
            verify_count=int(len(ver)), verify_sha=oracle.verify_stream_sha(ver["p"], ver["k"]),
            match_count=int(len(mt)), match_sha=mg.sha(mt.tobytes()),
            rules_matching=int(np.count_nonzero(hit)))
    with open(os.path.join(HERE, "lists.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
