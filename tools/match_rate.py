"""Cost of the match stage (yr_amd_match_device) on device-resident input.

    python tools/match_rate.py [--sets C,short] [--gib 1] [--reps 10] [--out profiles/match_rates.json]

Per rule set, on the same 1 GiB of the canonical xorshift input, one process,
median of --reps after a warm-up, HIP events on the scanner's stream around
each call (the calls are synchronous, so the bracket is the call):
  (a) yr_amd_verify_device alone;
  (a+b) yr_amd_match_device, which runs (a) underneath; (b) = the difference,
      reported as a fraction of (a);
  (c) what a caller without the stage does: D2H of all records, then the
      numpy filter / first-wins unique over (string, offset), on the host's
      clock.  (It has no lengths or xor keys yet: those need the block's bytes
      on the host as well, so (c) is a lower bound of the host path.)

    python tools/match_rate.py --hex [--gib 1] [--reps 10] [--out profiles/hex_match_rates.json]

The hex class (YR_AMD_MATCH_HEX) on config C: --gib of C's planted input
(tests/golden/planted.py) resident in HBM, one scan, then yr_amd_match_device
with the classes LITERAL and LITERAL | HEX alternating, medians of --reps after
a warm-up with min..max, HIP events around the synchronous call.  The added
cost is the difference of the medians.  What a caller without the class does
with the hex strings' records starts with their D2H (the rest of the LITERAL
call, almost all of them hex records), timed here on the host's clock; the
host's re-verification of every such record comes on top, so the D2H alone is
a LOWER BOUND of that path.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def hex_leg(a):
    import ctypes
    import numpy as np
    import torch
    import yara_amd
    from yara_amd import _hip, _lib
    sys.path[:0] = [os.path.join(REPO, "tests", "golden")]
    import gen_rules
    import oracle
    import planted
    n = int(a.gib * (1 << 30))
    host = planted.planted_buffer(oracle.xorshift, gen_rules.gen("C"), n, 3)
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    buf[:n] = torch.from_numpy(host).cuda()
    del host
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    path = os.path.join(REPO, "tests", "golden", "tables", "C.npz")
    z = np.load(path)
    t = yara_amd.Tables.from_npz(path, strings=True)
    LIT, BOTH = yara_amd.MATCH_LITERAL, yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX
    hex_strings = t.match_strings(BOTH) & ~t.match_strings(LIT)
    sc = yara_amd.Scanner(t, stream=stream.cuda_stream)
    sc.scan_device(buf.data_ptr(), n)
    _, cand, _ = sc.device_result()

    def stage(classes):   # (ms, n_matches, n_rest, rest pointer): the device call alone
        sc.set_match_classes(classes)
        pm, pr = ctypes.c_void_p(), ctypes.c_void_p()
        nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        _lib.check("yr_amd_match_device", _lib.lib().yr_amd_match_device(
            sc._h, 0, ctypes.byref(pm), ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr)))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), nm.value, nr.value, pr.value

    def d2h(ptr, cnt):
        t1 = time.perf_counter()
        recs = np.zeros(cnt, dtype=_lib.VERIFY_REC_DTYPE)
        if cnt:
            _hip.memcpy(recs.ctypes.data, ptr, cnt * 16, 2)
        return (time.perf_counter() - t1) * 1e3, recs

    for _ in range(2):   # warm-up: buffers grown, clocks up
        stage(LIT)
        stage(BOTH)
    lit, both, copy = [], [], []
    for _ in range(a.reps):   # interleaved
        ms, m_lit, r_lit, ptr = stage(LIT)
        lit.append(ms)
        c, recs = d2h(ptr, r_lit)
        copy.append(c)
        ms, m_both, r_both, _ = stage(BOTH)
        both.append(ms)
    _, records = sc.verify_device(0)
    hex_records = int(hex_strings[z["pool_string"][recs["pool_index"]]].sum())
    med = lambda v: round(statistics.median(v), 4)   # noqa: E731
    span = lambda v: [round(min(v), 4), round(max(v), 4)]   # noqa: E731
    out = {
        "input": "C planted (tests/golden/planted.py, seed 3)", "bytes": n, "reps": a.reps,
        "candidates": cand, "records": records,
        "literal": {"matches": m_lit, "rest": r_lit, "match_device_ms": med(lit),
                    "min_max_ms": span(lit)},
        "literal_hex": {"matches": m_both, "rest": r_both, "match_device_ms": med(both),
                        "min_max_ms": span(both)},
        "hex_records_in_literal_rest": hex_records,
        "added_ms": round(med(both) - med(lit), 4),
        "host_d2h_of_rest_ms": med(copy), "host_d2h_min_max_ms": span(copy),
        "host_d2h_is": "a lower bound of the path without the class: the host's "
                       "re-verification of the records is not included",
    }
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C,short")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hex", action="store_true",
                    help="the hex class on config C's planted input instead of the sets")
    a = ap.parse_args()
    if a.hex:
        return hex_leg(a)
    import numpy as np
    import torch
    import yara_amd
    from yara_amd import _hip, _lib
    n = int(a.gib * (1 << 30))
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    yara_amd.fill_xorshift64(buf.data_ptr(), n, 1)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    med = lambda v: round(statistics.median(v), 4)   # noqa: E731
    out = {"bytes": n, "reps": a.reps, "sets": {}}
    for name in a.sets.split(","):
        path = os.path.join(REPO, "tests", "golden", "tables", name + ".npz")
        z = np.load(path)
        t = yara_amd.Tables.from_npz(path, strings=True)
        final = t.final_strings()
        sc = yara_amd.Scanner(t, stream=stream.cuda_stream)
        sc.scan_device(buf.data_ptr(), n)
        _, cand, _ = sc.device_result()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), r

        def stage():   # (n_matches, n_rest): the device call alone, nothing copied
            import ctypes
            pm, pr = ctypes.c_void_p(), ctypes.c_void_p()
            nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
            _lib.check("yr_amd_match_device", _lib.lib().yr_amd_match_device(
                sc._h, 0, ctypes.byref(pm), ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr)))
            return nm.value, nr.value

        def host_path():
            ptr, cnt = sc.verify_device(0)
            t1 = time.perf_counter()
            recs = np.zeros(cnt, dtype=_lib.VERIFY_REC_DTYPE)
            _hip.memcpy(recs.ctypes.data, ptr, cnt * 16, 2)
            t2 = time.perf_counter()
            string = z["pool_string"][recs["pool_index"]]
            fin = final[string]
            rest = recs[~fin]
            key = string[fin].astype(np.uint64) << np.uint64(32) | recs["offset"][fin]
            _, first = np.unique(key, return_index=True)
            t3 = time.perf_counter()
            return (t2 - t1) * 1e3, (t3 - t2) * 1e3, len(first), len(rest)

        for _ in range(2):   # warm-up: buffers grown, clocks up
            sc.verify_device(0)
            stage()
            host_path()
        va, vb, d2h, host = [], [], [], []
        for _ in range(a.reps):   # interleaved
            ms, (_, nrec) = timed(lambda: sc.verify_device(0))
            va.append(ms)
            ms, (nm, nr) = timed(stage)
            vb.append(ms)
            c, h, hm, hr = host_path()
            d2h.append(c)
            host.append(h)
            assert (hm, hr) == (nm, nr), ((hm, hr), (nm, nr))
        a_ms, ab_ms = med(va), med(vb)
        out["sets"][name] = {
            "candidates": cand, "records": nrec, "matches": nm, "rest": nr,
            "verify_ms": a_ms, "match_device_ms": ab_ms, "stage_ms": round(ab_ms - a_ms, 4),
            "stage_over_verify": round((ab_ms - a_ms) / a_ms, 3),
            "host_d2h_ms": med(d2h), "host_numpy_ms": med(host),
            "host_path_ms": round(med(d2h) + med(host), 4),
            "verify_ms_all": [round(v, 4) for v in va], "match_device_ms_all": [round(v, 4) for v in vb],
        }
        print(name, json.dumps(out["sets"][name]), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
