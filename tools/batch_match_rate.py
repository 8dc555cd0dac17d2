"""Cost of the batch's match stage (yr_amd_match_batch_device) on an arena in HBM.

    python tools/batch_match_rate.py [--sets C,short] [--reps 10] [--buffers N] [--out profiles/batch_match_rates.json]

Per rule set and workload -- 65,536 buffers of 4 KiB and 4,096 buffers of
64 KiB of the canonical xorshift input, back to back in one device arena --
the batch is scanned once (yr_amd_scan_batch_device, yr_amd_scan_batch_result)
and then, medians of --reps interleaved repetitions after a warm-up with
min..max, HIP events on the scanner's stream around each synchronous call:
  (a)   yr_amd_verify_batch_device alone;
  (a+b) yr_amd_match_batch_device, which runs (a) underneath; (b) = the difference;
  (c)   what a caller had before the stage: D2H of all records, then per
        buffer the numpy filter and first-wins unique, vectorised over the
        batch (one stable lexsort by (buffer, string, offset)), on the host's
        clock.  No lengths or xor keys yet: (c) is a lower bound of that path.
  (d)   one yr_amd_scan_block_matches per buffer on --sample buffers (host
        bytes of the same input, wall clock), EXTRAPOLATED to the batch's
        buffer count -- reported as extrapolated, and it includes the scan,
        which (a)..(c) do not.

    python tools/batch_match_rate.py --hex [--reps 10] [--out profiles/batch_hex_match_rates.json]

The hex class of the batch stage (yr_amd_scanner_set_batch_match_classes) on
config C: C's planted input (tests/golden/planted.py, as tools/match_rate.py
--hex) resident in HBM, cut back to back into the same two workloads, scanned
once; then per batch, measured as above:
  (a)   yr_amd_match_batch_device with LITERAL: records -> matches, rest;
  (b)   the same with LITERAL | HEX: records -> items -> matches, rest; (b) -
        (a) is what the class costs;
  (c)   what a caller had for the same answer without the class: (a) plus the
        D2H of its rest records (host clock).  A LOWER BOUND: the host's
        re-verification of those records is not measured;
  (d)   one yr_amd_scan_block_matches with the hex class per buffer on the
        first --sample buffers, wall clock, EXTRAPOLATED by n / sample.
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

WORKLOADS = [(65536, 4 << 10), (4096, 64 << 10)]


def hex_leg(a):
    import numpy as np
    import torch
    import yara_amd
    from yara_amd import _hip, _lib
    sys.path[:0] = [os.path.join(REPO, "tests", "golden")]
    import gen_rules
    import oracle
    import planted
    L = _lib.lib()
    stream = torch.cuda.Stream()
    path = os.path.join(REPO, "tests", "golden", "tables", "C.npz")
    t = yara_amd.Tables.from_npz(path, strings=True)
    LIT, BOTH = yara_amd.MATCH_LITERAL, yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),   # noqa: E731
                      "max": round(max(v), 4)}
    out = {"input": "C planted (tests/golden/planted.py, seed 3)", "reps": a.reps,
           "sample": a.sample, "runs": []}
    host, buf = None, None
    for n, size in WORKLOADS:
        if a.buffers and n != a.buffers:
            continue
        n //= a.scale
        total = n * size
        if host is None or host.size != total:
            host = planted.planted_buffer(oracle.xorshift, gen_rules.gen("C"), total, 3)
            buf = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
            buf[:total] = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
        sizes = np.full(n, size, np.uint64)
        starts = np.arange(n, dtype=np.uint64) * np.uint64(size)
        sc = yara_amd.Scanner(t, stream=stream.cuda_stream)
        sc.scan_batch_device(buf.data_ptr(), total, starts, sizes)
        _, cand_off, _ = sc.batch_result()
        p1, p2 = ctypes.c_void_p(), ctypes.c_void_p()
        o1, o2 = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)()

        def stage(classes):   # (ms, matches, rest, rest pointer): the device call alone
            sc.set_batch_match_classes(classes)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check("yr_amd_match_batch_device", L.yr_amd_match_batch_device(
                sc._h, None, ctypes.byref(p1), ctypes.byref(o1), ctypes.byref(p2), ctypes.byref(o2)))
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), o1[n], o2[n], p2.value

        def d2h(ptr, cnt):
            t1 = time.perf_counter()
            recs = np.zeros(cnt, dtype=_lib.VERIFY_REC_DTYPE)
            if cnt:
                _hip.memcpy(recs.ctypes.data, ptr, cnt * 16, 2)
            return (time.perf_counter() - t1) * 1e3

        def singles():   # (d): the sample's per-buffer calls with the hex class, wall clock, in ms
            k = min(a.sample, n)
            ptrs = [ctypes.cast(host.ctypes.data + j * size, _lib._u8p) for j in range(k)]
            pm, pr = ctypes.POINTER(_lib.MatchRec)(), ctypes.POINTER(_lib.VerifyRec)()
            nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
            one = yara_amd.Scanner(t)
            one.set_match_classes(BOTH)
            for p in ptrs[:8]:   # warm-up
                L.yr_amd_scan_block_matches(one._h, p, size, 0, ctypes.byref(pm), ctypes.byref(nm),
                                            ctypes.byref(pr), ctypes.byref(nr))
            t0 = time.perf_counter()
            for p in ptrs:
                rc = L.yr_amd_scan_block_matches(one._h, p, size, 0, ctypes.byref(pm),
                                                 ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr))
                assert rc == 0
            ms = (time.perf_counter() - t0) * 1e3
            one.close()
            return k, ms

        for _ in range(2):   # warm-up: buffers grown, clocks up
            stage(LIT)
            stage(BOTH)
        lit, both, copy = [], [], []
        for _ in range(a.reps):   # interleaved
            ms, m_lit, r_lit, ptr = stage(LIT)
            lit.append(ms)
            copy.append(d2h(ptr, r_lit))
            ms, m_both, r_both, _ = stage(BOTH)
            both.append(ms)
        k, sample_ms = singles()
        med = statistics.median
        run = {
            "rules": "C", "buffers": n, "buffer_bytes": size, "candidates": int(cand_off[-1]),
            "literal": {"matches": int(m_lit), "rest": int(r_lit), "match_batch_ms": stat(lit)},
            "literal_hex": {"matches": int(m_both), "rest": int(r_both), "match_batch_ms": stat(both)},
            "added_ms": round(med(both) - med(lit), 4),
            "literal_rest_d2h_ms": stat(copy),
            "literal_plus_d2h_ms": round(med(lit) + med(copy), 4),
            "literal_plus_d2h_is": "a lower bound of the path without the class: the host's "
                                   "re-verification of the rest records is not included",
            "singles_sample": k, "singles_sample_ms": round(sample_ms, 3),
            "singles_extrapolated_ms": round(sample_ms * n / k, 1),
            "singles_is": "extrapolated from the sample by buffers / sample; includes the scans",
        }
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C,short")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--scale", type=int, default=1, help="divide the buffer counts (rehearsals)")
    ap.add_argument("--buffers", type=int, default=0, help="only the workload of this many buffers")
    ap.add_argument("--out", default=None)
    ap.add_argument("--hex", action="store_true",
                    help="the batch's hex class on config C's planted input instead of the sets")
    a = ap.parse_args()
    if a.hex:
        return hex_leg(a)
    import numpy as np
    import torch
    import yara_amd
    from yara_amd import _hip, _lib
    L = _lib.lib()
    stream = torch.cuda.Stream()
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),   # noqa: E731
                      "max": round(max(v), 4)}
    out = {"reps": a.reps, "sample": a.sample, "runs": []}
    for name in a.sets.split(","):
        path = os.path.join(REPO, "tests", "golden", "tables", name + ".npz")
        z = np.load(path)
        t = yara_amd.Tables.from_npz(path, strings=True)
        final = t.final_strings()
        for n, size in WORKLOADS:
            if a.buffers and n != a.buffers:
                continue
            n //= a.scale
            total = n * size
            buf = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
            yara_amd.fill_xorshift64(buf.data_ptr(), total, 1)
            torch.cuda.synchronize()
            sizes = np.full(n, size, np.uint64)
            starts = np.arange(n, dtype=np.uint64) * np.uint64(size)
            sc = yara_amd.Scanner(t, stream=stream.cuda_stream)
            sc.scan_batch_device(buf.data_ptr(), total, starts, sizes)
            _, cand_off, _ = sc.batch_result()
            p1, p2 = ctypes.c_void_p(), ctypes.c_void_p()
            o1, o2 = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)()

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r = fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), r

            def verify():   # the device call alone, nothing copied
                _lib.check("yr_amd_verify_batch_device", L.yr_amd_verify_batch_device(
                    sc._h, None, ctypes.byref(p1), ctypes.byref(o1)))
                return o1[n]

            def stage():
                _lib.check("yr_amd_match_batch_device", L.yr_amd_match_batch_device(
                    sc._h, None, ctypes.byref(p1), ctypes.byref(o1), ctypes.byref(p2),
                    ctypes.byref(o2)))
                return o1[n], o2[n]

            def host_path():
                nrec = verify()
                rec_off = np.ctypeslib.as_array(o1, shape=(n + 1,)).copy()
                t1 = time.perf_counter()
                recs = np.zeros(nrec, dtype=_lib.VERIFY_REC_DTYPE)
                _hip.memcpy(recs.ctypes.data, p1.value, nrec * 16, 2)
                t2 = time.perf_counter()
                b = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rec_off.astype(np.int64)))
                string = z["pool_string"][recs["pool_index"]]
                fin = final[string]
                rest = recs[~fin]
                s, o, b = string[fin], recs["offset"][fin], b[fin]
                order = np.lexsort((o, s, b))
                s, o, b = s[order], o[order], b[order]
                keep = np.ones(s.size, bool)
                keep[1:] = (b[1:] != b[:-1]) | (s[1:] != s[:-1]) | (o[1:] != o[:-1])
                t3 = time.perf_counter()
                return (t2 - t1) * 1e3, (t3 - t2) * 1e3, int(keep.sum()), len(rest)

            def singles():   # (d): the sample's per-buffer calls, wall clock, in ms
                k = min(a.sample, n)
                host = buf[:k * size].cpu().numpy()
                ptrs = [ctypes.cast(host.ctypes.data + j * size, _lib._u8p) for j in range(k)]
                pm, pr = ctypes.POINTER(_lib.MatchRec)(), ctypes.POINTER(_lib.VerifyRec)()
                nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
                one = yara_amd.Scanner(t)
                for p in ptrs[:8]:   # warm-up
                    L.yr_amd_scan_block_matches(one._h, p, size, 0, ctypes.byref(pm), ctypes.byref(nm),
                                                ctypes.byref(pr), ctypes.byref(nr))
                t0 = time.perf_counter()
                for p in ptrs:
                    rc = L.yr_amd_scan_block_matches(one._h, p, size, 0, ctypes.byref(pm),
                                                     ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr))
                    assert rc == 0
                ms = (time.perf_counter() - t0) * 1e3
                one.close()
                return k, ms

            for _ in range(2):   # warm-up: buffers grown, clocks up
                verify()
                stage()
                host_path()
            va, vb, d2h, host = [], [], [], []
            for _ in range(a.reps):   # interleaved
                ms, nrec = timed(verify)
                va.append(ms)
                ms, (nm, nr) = timed(stage)
                vb.append(ms)
                c, h, hm, hr = host_path()
                d2h.append(c)
                host.append(h)
                assert (hm, hr) == (nm, nr), ((hm, hr), (nm, nr))
            k, sample_ms = singles()
            run = {
                "rules": name, "buffers": n, "buffer_bytes": size, "candidates": int(cand_off[-1]),
                "records": int(nrec), "matches": int(nm), "rest": int(nr),
                "verify_batch_ms": stat(va), "match_batch_ms": stat(vb),
                "stage_ms": round(statistics.median(vb) - statistics.median(va), 4),
                "host_d2h_ms": stat(d2h), "host_numpy_ms": stat(host),
                "host_path_ms": round(statistics.median(d2h) + statistics.median(host), 4),
                "singles_sample": k, "singles_sample_ms": round(sample_ms, 3),
                "singles_extrapolated_ms": round(sample_ms * n / k, 1),
            }
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
            sc.close()
            del buf
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
