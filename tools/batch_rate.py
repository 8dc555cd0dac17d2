"""Rate of many small host buffers: what batching buys (not the bench metric).

Config C tables on the canonical xorshift input, two workloads of 256 MiB each
-- 4,096 buffers of 64 KiB and 65,536 buffers of 4 KiB -- through three paths,
records fetched to the host in each (the replay is the caller's, not timed):
  loop      yr_amd_scan_block_verified, one call per buffer
  pipeline  yr_amd_pipeline_submit / _next at depth 8
  batch     yr_amd_scan_batch_verified, one call for the whole list
Every path goes straight through the C ABI (raw ctypes calls on prepared
pointers: a few microseconds of Python per call, against the tens to hundreds
of microseconds a block costs).  5 repetitions, the three paths interleaved in
each; medians and min..max spreads of buffers/s and GB/s.

    python tools/batch_rate.py [--reps 5] [--out profiles/batch_rates.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

WORKLOADS = [(4096, 64 << 10), (65536, 4 << 10)]
DEPTH = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rules", default="C")
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=int, default=1, help="divide the buffer counts (rehearsals)")
    a = ap.parse_args()
    import torch
    import oracle
    import yara_amd
    from yara_amd import _lib
    from conftest import tables_npz
    assert torch.cuda.is_available(), "batch_rate.py measures on the GPU"
    L = _lib.lib()
    tab = yara_amd.Tables.from_npz(tables_npz(a.rules), device=0, strings=True)
    sc = yara_amd.Scanner(tab)
    pipe = yara_amd.Pipeline(tab, depth=DEPTH)
    rec = ctypes.POINTER(_lib.VerifyRec)()
    cnt = ctypes.c_uint64()
    off = ctypes.POINTER(ctypes.c_uint64)()
    pd, ps, pb = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(), ctypes.c_uint64()
    res = {"rules": a.rules, "reps": a.reps, "pipeline_depth": DEPTH, "workloads": []}

    for n, size in WORKLOADS:
        n //= a.scale
        data = oracle.xorshift(n * size, 1)
        base = data.ctypes.data
        ptrs = [ctypes.cast(base + k * size, _lib._u8p) for k in range(n)]
        parr = (ctypes.c_void_p * n)(*[base + k * size for k in range(n)])
        sarr = (ctypes.c_size_t * n)(*([size] * n))

        def loop():
            tot = 0
            for p in ptrs:
                rc = L.yr_amd_scan_block_verified(sc._h, p, size, 0, ctypes.byref(rec), ctypes.byref(cnt))
                assert rc == 0
                tot += cnt.value
            return tot

        def nxt():
            rc = L.yr_amd_pipeline_next(pipe._h, ctypes.byref(rec), ctypes.byref(cnt), ctypes.byref(pd),
                                        ctypes.byref(ps), ctypes.byref(pb))
            assert rc == 0
            return cnt.value

        def pipeline():
            tot, inflight = 0, 0
            for p in ptrs:
                if inflight == DEPTH:
                    tot += nxt()
                    inflight -= 1
                assert L.yr_amd_pipeline_submit(pipe._h, p, size, 0) == 0
                inflight += 1
            while inflight:
                tot += nxt()
                inflight -= 1
            return tot

        def batch():
            rc = L.yr_amd_scan_batch_verified(sc._h, parr, sarr, None, n, ctypes.byref(rec),
                                              ctypes.byref(off))
            assert rc == 0
            return off[n]

        paths = [("loop", loop), ("pipeline", pipeline), ("batch", batch)]
        want = loop()           # warm-up of every path, and the records must agree
        assert pipeline() == want and batch() == want
        secs = {name: [] for name, _ in paths}
        for _ in range(a.reps):
            for name, fn in paths:   # interleaved
                t0 = time.perf_counter()
                got = fn()
                secs[name].append(time.perf_counter() - t0)
                assert got == want
        w = {"buffers": n, "buffer_bytes": size, "records": int(want), "paths": {}}
        for name, _ in paths:
            t = sorted(secs[name])
            med = statistics.median(t)
            w["paths"][name] = {
                "seconds": [round(x, 5) for x in secs[name]],
                "buffers_per_s_median": round(n / med),
                "buffers_per_s_spread": [round(n / t[-1]), round(n / t[0])],
                "GBps_median": round(n * size / med / 1e9, 3),
                "GBps_spread": [round(n * size / t[-1] / 1e9, 3), round(n * size / t[0] / 1e9, 3)],
            }
        # the batch path wins where its slowest run beats the others' fastest
        w["batch_beats_both_beyond_spread"] = all(
            max(secs["batch"]) < min(secs[o]) for o in ("loop", "pipeline"))
        res["workloads"].append(w)
        print(json.dumps(w), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
