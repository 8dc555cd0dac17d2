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

    python tools/batch_match_rate.py --hex-wide [--reps 10] [--out profiles/batch_hex_wide_rates.json]

The batch's wave-wide path (yr_amd_scanner_set_batch_hex_wide), classes
LITERAL | HEX, 256 MiB cut into the same two workloads, the setting off and on
alternating in one process, medians of --reps after a warm-up with min..max:
  - C's planted input under C's tables: nothing is queued, on - off is what the
    setting costs when idle (to be read against the off leg's own spread);
  - zeros with the hexwide fixture's `back` plant ({ B5 [0-100] B1 B2 B3 B4 },
    101 matches) once per buffer under the fixture's tables: on - off per wide
    record;
  - what a caller had for the second input before: one yr_amd_scan_block_matches
    with yr_amd_scanner_set_hex_wide(1) per buffer on the first --sample
    buffers, wall clock, EXTRAPOLATED by n / sample.

    python tools/batch_match_rate.py --alternations [--reps 10] [--parent-tree DIR --rounds 5]
                                     [--out profiles/batch_alternation_match_rates.json]

The batch's alternation strings (yr_amd_scanner_set_batch_alternations), classes
LITERAL | HEX, 256 MiB of rx's planted input (as tools/match_rate.py
--alternations) cut into the same two workloads: the setting off and on
alternating in one process, medians with min..max, matches and rest for both.
With --parent-tree the setting is left off and the same calls are timed on this
tree's library and on another build's (the parent commit's), one child process
each, alternating --rounds times: the idle cost of the change next to the
run-to-run spread the same runs show.

    python tools/batch_match_rate.py --loops [--reps 10] [--parent-tree DIR --rounds 5]
                                     [--out profiles/batch_loop_match_rates.json]

The batch's loop strings (yr_amd_scanner_set_batch_loops) in the same way, with a
third workload of 262,144 x 1 KiB (the loop waves' table is sized to the largest
buffer) and a second input: 65,536 `Rn6!a..z` records of the loops fixture's
`run` string (tools/match_rate.py planted_runs) under that fixture's tables, as
1 KiB and as 4 KiB buffers -- a queue 32 times the fixed grid at two table sizes.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (YARA_AMD_PACKAGE_ROOT: another build's yara_amd package with its library, --parent-tree's child)
sys.path.insert(0, os.environ.get("YARA_AMD_PACKAGE_ROOT") or REPO)

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


def hex_wide_leg(a):
    import numpy as np
    import torch
    import yara_amd
    from yara_amd import _lib
    sys.path[:0] = [os.path.join(REPO, "tests", "golden")]
    import gen_rules
    import oracle
    import planted
    L = _lib.lib()
    stream = torch.cuda.Stream()
    BOTH = yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),   # noqa: E731
                      "max": round(max(v), 4)}
    golden = os.path.join(REPO, "tests", "golden")
    total = (256 << 20) // a.scale
    out = {"bytes": total, "reps": a.reps, "sample": a.sample, "runs": []}
    for name, path in (("C planted", os.path.join(golden, "tables", "C.npz")),
                       ("back plant per buffer", os.path.join(golden, "hexwide", "tables.npz"))):
        t = yara_amd.Tables.from_npz(path, strings=True)
        for n, size in WORKLOADS:
            if a.buffers and n != a.buffers:
                continue
            n = total // size
            if name == "C planted":
                host = planted.planted_buffer(oracle.xorshift, gen_rules.gen("C"), total, 3)
            else:   # B5 at every depth 1..101 before the atom, as the fixture's `back` plant
                host = np.zeros((n, size), np.uint8)
                host[:, 256 - 101:256] = 0xB5
                host[:, 256:260] = (0xB1, 0xB2, 0xB3, 0xB4)
                host = host.reshape(-1)
            buf = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
            buf[:total] = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            sizes = np.full(n, size, np.uint64)
            starts = np.arange(n, dtype=np.uint64) * np.uint64(size)
            sc = yara_amd.Scanner(t, stream=stream.cuda_stream)
            sc.set_batch_match_classes(BOTH)
            sc.scan_batch_device(buf.data_ptr(), total, starts, sizes)
            sc.batch_result()
            p1, p2 = ctypes.c_void_p(), ctypes.c_void_p()
            o1, o2 = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)()

            def stage(wide):   # (ms, matches, rest): the device call alone
                sc.set_batch_hex_wide(wide)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                _lib.check("yr_amd_match_batch_device", L.yr_amd_match_batch_device(
                    sc._h, None, ctypes.byref(p1), ctypes.byref(o1), ctypes.byref(p2), ctypes.byref(o2)))
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), int(o1[n]), int(o2[n])

            for _ in range(2):   # warm-up: buffers and the queue grown, clocks up
                stage(False)
                stage(True)
            ms, count = {False: [], True: []}, {}
            for _ in range(a.reps):   # alternating
                for wide in (False, True):
                    v, m, r = stage(wide)
                    ms[wide].append(v)
                    count[wide] = (m, r)
            med = statistics.median
            wide_records = count[False][1] - count[True][1]
            run = {"input": name, "buffers": n, "buffer_bytes": size,
                   "off": {"matches": count[False][0], "rest": count[False][1], "ms": stat(ms[False])},
                   "on": {"matches": count[True][0], "rest": count[True][1], "ms": stat(ms[True])},
                   "on_minus_off_ms": round(med(ms[True]) - med(ms[False]), 4),
                   "wide_records": wide_records}
            if wide_records:
                run["us_per_wide_record"] = round(1e3 * run["on_minus_off_ms"] / wide_records, 4)
                k = min(a.sample, n)   # the path before: a single-block wide call per buffer
                ptrs = [ctypes.cast(host.ctypes.data + j * size, _lib._u8p) for j in range(k)]
                pm, pr = ctypes.POINTER(_lib.MatchRec)(), ctypes.POINTER(_lib.VerifyRec)()
                nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
                one = yara_amd.Scanner(t)
                one.set_match_classes(BOTH)
                one.set_hex_wide(True)
                for warm in (True, False):
                    t0 = time.perf_counter()
                    for p in ptrs[:8] if warm else ptrs:
                        rc = L.yr_amd_scan_block_matches(one._h, p, size, 0, ctypes.byref(pm),
                                                         ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr))
                        assert rc == 0
                    sample_ms = (time.perf_counter() - t0) * 1e3
                one.close()
                run.update({"singles_sample": k, "singles_sample_ms": round(sample_ms, 3),
                            "singles_extrapolated_ms": round(sample_ms * n / k, 1),
                            "singles_is": "extrapolated from the sample by buffers / sample; "
                                          "includes the scans"})
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
            sc.close()
            del buf
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def alternations_leg(a, mode="alternations"):
    import subprocess
    med = lambda v: round(statistics.median(v), 4)   # noqa: E731
    span = lambda v: [round(min(v), 4), round(max(v), 4)]   # noqa: E731
    total = (256 << 20) // a.scale
    if a.parent_tree and not a.child:
        out = {"bytes": total, "reps": a.reps, "rounds": a.rounds, "runs": []}
        sides = {"this": None, "parent": os.path.abspath(a.parent_tree)}
        meds = {}
        for _ in range(a.rounds):
            for side, lib in sides.items():
                env = dict(os.environ)
                if lib:
                    env["YARA_AMD_PACKAGE_ROOT"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--" + mode, "--child",
                                    "--reps", str(a.reps), "--scale", str(a.scale), "--buffers",
                                    str(a.buffers)], env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:   # (nothing more is started on the device)
                    sys.exit("child (%s) failed with %d:\n%s" % (side, r.returncode, r.stderr[-2000:]))
                ms = json.loads(r.stdout.strip().splitlines()[-1])["off_ms"]
                out["runs"].append({"side": side, "off_ms": ms})
                for k, v in ms.items():
                    meds.setdefault(k, {s: [] for s in sides})[side].append(v)
        out["idle"] = {k: {"this_median_ms": med(v["this"]), "this_min_max_ms": span(v["this"]),
                           "parent_median_ms": med(v["parent"]), "parent_min_max_ms": span(v["parent"]),
                           "this_over_parent": round(med(v["this"]) / med(v["parent"]), 4)}
                       for k, v in meds.items()}
        print(json.dumps(out["idle"]), flush=True)
    else:
        import numpy as np
        import torch
        import yara_amd
        from yara_amd import _lib
        sys.path[:0] = [os.path.join(REPO, "tests", "golden")]
        sys.path.append(REPO)   # (oracle; behind a --parent-tree package root)
        import oracle
        import planted
        L = _lib.lib()
        stream = torch.cuda.Stream()
        golden = os.path.join(REPO, "tests", "golden")
        out = {"bytes": total, "reps": a.reps, "classes": "LITERAL | HEX", "input": "rx planted", "runs": []}
        child = {}
        # (input, tables, its bytes, the buffer sizes it is cut into)
        legs = [("rx planted", os.path.join(golden, "tables", "rx.npz"),
                 lambda: planted.rx_buffer(oracle.xorshift, total, 19),   # (rx_1M's generator at this size)
                 [size for _, size in WORKLOADS] + ([1 << 10] if mode == "loops" and not a.child else []))]
        if mode == "loops" and not a.child:
            from match_rate import planted_runs
            legs.append(("65536 planted Rn6!a..z records", os.path.join(golden, "loops", "tables.npz"),
                         lambda: planted_runs(65536)[:65536 * 16], [1 << 10, 4 << 10]))
        for name, path, make, cuts in legs:
            t = yara_amd.Tables.from_npz(path, strings=True)
            host = make()
            nbytes = host.size
            buf = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
            buf[:nbytes] = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            for size in cuts:
                n = nbytes // size
                if a.buffers and dict(WORKLOADS).get(a.buffers) != size:
                    continue
                sizes = np.full(n, size, np.uint64)
                starts = np.arange(n, dtype=np.uint64) * np.uint64(size)
                sc = yara_amd.Scanner(t, stream=stream.cuda_stream)
                sc.set_batch_match_classes(yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX)
                sc.scan_batch_device(buf.data_ptr(), nbytes, starts, sizes)
                sc.batch_result()
                p1, p2 = ctypes.c_void_p(), ctypes.c_void_p()
                o1, o2 = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)()

                def stage(on):   # (ms, matches, rest): the device call alone
                    if on is not None:
                        getattr(sc, "set_batch_" + mode)(on)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    _lib.check("yr_amd_match_batch_device", L.yr_amd_match_batch_device(
                        sc._h, None, ctypes.byref(p1), ctypes.byref(o1), ctypes.byref(p2), ctypes.byref(o2)))
                    e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1), int(o1[n]), int(o2[n])

                if a.child:   # the setting is never touched: the same calls on either library
                    for _ in range(3):
                        stage(None)
                    child["%dx%d" % (n, size)] = med([stage(None)[0] for _ in range(a.reps)])
                    sc.close()
                    continue
                for _ in range(2):   # warm-up: buffers and the queue grown, clocks up
                    stage(False)
                    stage(True)
                ms, count = {False: [], True: []}, {}
                for _ in range(a.reps):   # alternating
                    for on in (False, True):
                        v, m, r = stage(on)
                        ms[on].append(v)
                        count[on] = (m, r)
                run = {"input": name, "buffers": n, "buffer_bytes": size,
                       "records": int(sc.verify_batch_device()[1][-1]),
                       "off": {"matches": count[False][0], "rest": count[False][1],
                               "match_batch_ms": med(ms[False]), "min_max_ms": span(ms[False])},
                       "on": {"matches": count[True][0], "rest": count[True][1],
                              "match_batch_ms": med(ms[True]), "min_max_ms": span(ms[True])},
                       "added_ms": round(med(ms[True]) - med(ms[False]), 4),
                       mode[:-1] + "_records": count[False][1] - count[True][1]}
                out["runs"].append(run)
                print(json.dumps(run), flush=True)
                sc.close()
        if a.child:
            print(json.dumps({"off_ms": child}), flush=True)
            return
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
    ap.add_argument("--hex-wide", action="store_true",
                    help="the batch's wave-wide path, off against on (see above)")
    ap.add_argument("--alternations", action="store_true",
                    help="the batch's alternation strings, off against on, on rx's planted input")
    ap.add_argument("--loops", action="store_true",
                    help="the batch's loop strings, off against on, on rx's planted input and on "
                         "planted records of the loops fixture's `run` string")
    ap.add_argument("--parent-tree", default=None,
                    help="with --alternations or --loops: a directory holding another build's yara_amd package "
                         "(the parent commit's, with its library) to time the setting off against, "
                         "alternating child processes")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.alternations or a.loops:
        return alternations_leg(a, "loops" if a.loops else "alternations")
    if a.hex_wide:
        return hex_wide_leg(a)
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
