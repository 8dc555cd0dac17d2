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

--gather measures instead the same two workloads DEVICE-resident: the buffers
lie in one torch allocation at pseudo-random odd byte offsets, records fetched
to the host in each leg:
  gather    yr_amd_scan_batch_gather_device, one call for the whole list
  memcpy    what a caller could write without it: one hipMemcpyDtoDAsync per
            buffer into a yr_amd_batch_layout arena (allocated beforehand),
            then yr_amd_scan_batch_device
and, by device events, yr_amd_batch_gather alone (its table upload and the
kernel) next to ONE hipMemcpyDtoDAsync of the same bytes, in GB/s of payload.

    python tools/batch_rate.py --gather [--reps 5] [--out profiles/batch_gather_rates.json]
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
    ap.add_argument("--gather", action="store_true", help="the device-resident legs")
    a = ap.parse_args()
    if a.gather:
        return gather_main(a)
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


def _spread(secs, n, size):
    t = sorted(secs)
    med = statistics.median(t)
    return {
        "seconds": [round(x, 5) for x in secs],
        "buffers_per_s_median": round(n / med),
        "buffers_per_s_spread": [round(n / t[-1]), round(n / t[0])],
        "GBps_median": round(n * size / med / 1e9, 3),
        "GBps_spread": [round(n * size / t[-1] / 1e9, 3), round(n * size / t[0] / 1e9, 3)],
    }


def gather_main(a):
    import numpy as np
    import torch
    import oracle
    import yara_amd
    from yara_amd import _hip, _lib
    from conftest import tables_npz
    assert torch.cuda.is_available(), "batch_rate.py measures on the GPU"
    L = _lib.lib()
    H = _hip.hip()
    H.hipMemcpyDtoDAsync.restype = ctypes.c_int
    H.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    u64p = lambda x: x.ctypes.data_as(_lib._u64p)   # noqa: E731
    tab = yara_amd.Tables.from_npz(tables_npz(a.rules), device=0, strings=True)
    # every leg's work on ONE stream, the scanner's: the copies of the memcpy leg too
    stream = torch.cuda.Stream()
    sh = ctypes.c_void_p(stream.cuda_stream)
    sc = yara_amd.Scanner(tab, stream=stream.cuda_stream)
    d_rec = ctypes.c_void_p()
    off = ctypes.POINTER(ctypes.c_uint64)()
    res = {"rules": a.rules, "reps": a.reps, "workloads": []}

    for n, size in WORKLOADS:
        n //= a.scale
        data = oracle.xorshift(n * size, 1)
        # buffer k at the odd offset k * (size + 16) + {1, 3, .., 15}
        rng = np.random.default_rng(5)
        odd = 2 * rng.integers(0, 8, n) + 1
        pitch = size + 16
        img = np.full(n * pitch + 16, 0xA5, np.uint8)
        rows = img[:n * pitch].reshape(n, pitch)
        for o in range(1, 16, 2):
            sel = np.flatnonzero(odd == o)
            rows[sel, o:o + size] = data.reshape(n, size)[sel]
        src = torch.from_numpy(img).cuda()
        offs = np.arange(n, dtype=np.uint64) * np.uint64(pitch) + odd.astype(np.uint64)
        ptrs = np.uint64(src.data_ptr()) + offs
        assert np.all(ptrs % 2 == 1)
        sizes = np.full(n, size, np.uint64)
        starts, arena_size = yara_amd.batch_layout(sizes)
        arena = torch.empty(arena_size + 16, dtype=torch.uint8, device="cuda")
        whole = torch.empty(n * size, dtype=torch.uint8, device="cuda")   # (the one-copy yardstick)
        hrec = np.zeros(1 << 16, dtype=_lib.VERIFY_REC_DTYPE)
        torch.cuda.synchronize()
        plist, slist = [int(p) for p in ptrs], [int(arena.data_ptr()) + int(s) for s in starts]

        def finish():
            nonlocal hrec
            assert L.yr_amd_scan_batch_result(sc._h, None, None, None) == 0
            assert L.yr_amd_verify_batch_device(sc._h, None, ctypes.byref(d_rec), ctypes.byref(off)) == 0
            tot = off[n]
            if tot > hrec.size:
                hrec = np.zeros(2 * tot, dtype=_lib.VERIFY_REC_DTYPE)
            _hip.memcpy(hrec.ctypes.data, d_rec.value or 0, tot * 16, 2)
            return tot

        def gather():
            assert L.yr_amd_scan_batch_gather_device(sc._h, u64p(ptrs), u64p(sizes), n) == 0
            return finish()

        def memcpy():
            for d, s in zip(slist, plist):
                assert H.hipMemcpyDtoDAsync(d, s, size, sh) == 0
            assert L.yr_amd_scan_batch_device(sc._h, arena.data_ptr(), arena_size, u64p(starts),
                                              u64p(sizes), n) == 0
            return finish()

        # the records must be those of the host batch path on the same bytes
        want = len(sc.batch_verify_calls(list(data.reshape(n, size)))[0])
        paths = [("gather", gather), ("memcpy", memcpy)]
        assert gather() == want and memcpy() == want   # (warm-up)
        secs = {name: [] for name, _ in paths}
        for _ in range(a.reps):
            for name, fn in paths:   # interleaved
                t0 = time.perf_counter()
                got = fn()
                secs[name].append(time.perf_counter() - t0)
                assert got == want
        w = {"buffers": n, "buffer_bytes": size, "records": int(want),
             "paths": {name: _spread(secs[name], n, size) for name, _ in paths}}
        w["gather_beats_memcpy_beyond_spread"] = max(secs["gather"]) < min(secs["memcpy"])

        # the gather alone (table upload + kernel) and one copy of the same bytes
        def gather_only():
            assert L.yr_amd_batch_gather(sc._h, arena.data_ptr(), arena_size, u64p(starts), u64p(ptrs),
                                         u64p(sizes), n) == 0

        def one_copy():
            assert H.hipMemcpyDtoDAsync(whole.data_ptr(), src.data_ptr(), n * size, sh) == 0

        ms = {"gather": [], "one_copy": []}
        for rep in range(a.reps + 1):
            for name, fn in (("gather", gather_only), ("one_copy", one_copy)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if rep > 0:   # (the first round warms up)
                    ms[name].append(e0.elapsed_time(e1))
        gb = lambda x: round(n * size / (x * 1e-3) / 1e9, 1)   # noqa: E731
        w["gather_alone"] = {k: {"ms": [round(x, 4) for x in v], "GBps_median": gb(statistics.median(v)),
                                 "GBps_spread": [gb(max(v)), gb(min(v))]} for k, v in ms.items()}
        w["gather_alone"]["fraction_of_one_copy"] = round(
            statistics.median(ms["one_copy"]) / statistics.median(ms["gather"]), 3)
        res["workloads"].append(w)
        print(json.dumps(w), flush=True)
        del src, arena, whole
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
