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

    python tools/match_rate.py --hex-wide [--gib 1] [--reps 10] [--out profiles/hex_wide_rates.json]

The wave-wide path (yr_amd_scanner_set_hex_wide), classes LITERAL | HEX, the
setting off and on alternating in one process, medians of --reps after a
warm-up with min..max.  Two inputs of --gib: config C's planted input, whose
rules hold no jump wider than 63 -- no record is queued, the difference is what
the setting costs by itself (four launches more) -- and zeros with 4096 copies
of the hexwide fixture's `back` string ({ B5 [0-100] B1 B2 B3 B4 }, 1 to 100
starts each) under that fixture's tables: every record is wide, the difference
over the records is the time per wide record.  The D2H of the rest with the
setting off is again the lower bound of what a caller does without it.

    python tools/match_rate.py --alternations [--gib 1] [--reps 10] [--parent-tree DIR --rounds 5]
                               [--out profiles/alternation_match_rates.json]

Alternation strings (yr_amd_scanner_set_alternations), classes LITERAL | HEX, on
rx's planted input: the setting off and on alternating in one process, medians
with min..max, records -> matches and rest for both.  With --parent-tree the
setting is left off and the same calls are timed on this tree's library and on
another build's (the parent commit's), one child process each, alternating
--rounds times: the idle cost of the change next to the run-to-run spread the
same runs show.

    python tools/match_rate.py --loops [--gib 1] [--reps 10] [--out profiles/loop_match_rates.json]

Loop strings (yr_amd_scanner_set_loops) in the same way, on two inputs: rx's
planted input under rx's tables (its string 4 is a loop string), and 65,536
`Rn6!a..z` records, one every 16 bytes of 1 MiB of zeros, under the tables of
tests/golden/loops -- a queue 32 times the fixed grid, every record settled.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (YARA_AMD_PACKAGE_ROOT: another build's yara_amd package with its library, --parent-tree's child)
sys.path.insert(0, os.environ.get("YARA_AMD_PACKAGE_ROOT") or REPO)


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


def hex_wide_leg(a):
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
    golden = os.path.join(REPO, "tests", "golden")
    stream = torch.cuda.Stream()
    med = lambda v: round(statistics.median(v), 4)   # noqa: E731
    span = lambda v: [round(min(v), 4), round(max(v), 4)]   # noqa: E731
    out = {"bytes": n, "reps": a.reps, "classes": "LITERAL | HEX", "inputs": {}}
    for name in ("C planted", "hexwide planted"):
        if name == "C planted":
            host = planted.planted_buffer(oracle.xorshift, gen_rules.gen("C"), n, 3)
            path = os.path.join(golden, "tables", "C.npz")
        else:
            host = np.zeros(n, np.uint8)
            for k in range(4096):   # B5 x (1 + k % 100), then the atom
                at = (k + 1) * (n // 4100)
                host[at - 1 - k % 100:at] = 0xB5
                host[at:at + 4] = (0xB1, 0xB2, 0xB3, 0xB4)
            path = os.path.join(golden, "hexwide", "tables.npz")
        buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        buf[:n] = torch.from_numpy(host).cuda()
        del host
        torch.cuda.synchronize()
        sc = yara_amd.Scanner(yara_amd.Tables.from_npz(path, strings=True),
                              stream=stream.cuda_stream)
        sc.set_match_classes(yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX)
        sc.scan_device(buf.data_ptr(), n)
        sc.device_result()

        def stage(wide):   # (ms, n_matches, n_rest, rest pointer): the device call alone
            sc.set_hex_wide(wide)
            pm, pr = ctypes.c_void_p(), ctypes.c_void_p()
            nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check("yr_amd_match_device", _lib.lib().yr_amd_match_device(
                sc._h, 0, ctypes.byref(pm), ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr)))
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), nm.value, nr.value, pr.value

        for _ in range(2):   # warm-up: buffers grown, clocks up
            stage(False)
            stage(True)
        off, on, copy = [], [], []
        for _ in range(a.reps):   # interleaved
            ms, m_off, r_off, ptr = stage(False)
            off.append(ms)
            t1 = time.perf_counter()
            recs = np.zeros(r_off, dtype=_lib.VERIFY_REC_DTYPE)
            if r_off:
                _hip.memcpy(recs.ctypes.data, ptr, r_off * 16, 2)
            copy.append((time.perf_counter() - t1) * 1e3)
            ms, m_on, r_on, _ = stage(True)
            on.append(ms)
        wide_records = r_off - r_on
        out["inputs"][name] = {
            "records": sc.verify_device(0)[1],
            "off": {"matches": m_off, "rest": r_off, "match_device_ms": med(off),
                    "min_max_ms": span(off)},
            "on": {"matches": m_on, "rest": r_on, "match_device_ms": med(on),
                   "min_max_ms": span(on)},
            "added_ms": round(med(on) - med(off), 4), "wide_records": wide_records,
            "us_per_wide_record": round((med(on) - med(off)) * 1e3 / wide_records, 4)
            if wide_records else None,
            "host_d2h_of_rest_off_ms": med(copy), "host_d2h_min_max_ms": span(copy),
        }
        print(name, json.dumps(out["inputs"][name]), flush=True)
        sc.close()
        del buf
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def planted_runs(records):
    """`Rn6!a..z` of tests/golden/loops' string `run`, one record every 16 bytes of zeros."""
    import numpy as np
    buf = np.zeros(records * 16 + 64, np.uint8)
    rows = buf[:records * 16].reshape(records, 16)
    for k in range(7):   # Rn6! + 1..7 a + z
        word = np.frombuffer(b"Rn6!" + b"a" * (1 + k) + b"z", np.uint8)
        rows[k::7, 4:4 + word.size] = word
    return buf


def alternations_leg(a, mode="alternations"):
    """yr_amd_match_device on rx's planted input resident in HBM, classes LITERAL | HEX, the
    alternation setting (mode "loops": the loop setting; then a second input, planted_runs
    under the loops fixture's tables) off and on, alternating.  With --parent-tree: the setting OFF on this
    tree's library and on another build's (the parent commit's), one child process each,
    alternating, a.rounds times -- the idle cost of the change against its run-to-run spread."""
    import ctypes
    import subprocess
    import numpy as np
    med = lambda v: round(statistics.median(v), 4)   # noqa: E731
    span = lambda v: [round(min(v), 4), round(max(v), 4)]   # noqa: E731
    if a.parent_tree and not a.child:
        out = {"bytes": int(a.gib * (1 << 30)), "reps": a.reps, "rounds": a.rounds, "runs": []}
        sides = {"this": None, "parent": os.path.abspath(a.parent_tree)}
        meds = {k: [] for k in sides}
        for _ in range(a.rounds):
            for side, lib in sides.items():
                env = dict(os.environ)
                if lib:
                    env["YARA_AMD_PACKAGE_ROOT"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--" + mode,
                                    "--child", "--gib", str(a.gib), "--reps", str(a.reps)],
                                   env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:   # (nothing more is started on the device)
                    sys.exit("child (%s) failed with %d:\n%s" % (side, r.returncode, r.stderr[-2000:]))
                ms = json.loads(r.stdout.strip().splitlines()[-1])["off_ms"]
                meds[side].append(ms)
                out["runs"].append({"side": side, "off_ms": ms})
        out["idle"] = {k: {"median_ms": med(v), "min_max_ms": span(v)} for k, v in meds.items()}
        out["idle"]["this_over_parent"] = round(med(meds["this"]) / med(meds["parent"]), 4)
        out["idle"]["spread"] = {k: round((max(v) - min(v)) / med(v), 4) for k, v in meds.items()}
        print(json.dumps(out["idle"]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        return
    import torch
    import yara_amd
    from yara_amd import _lib
    sys.path[:0] = [os.path.join(REPO, "tests", "golden")]
    sys.path.append(REPO)   # (oracle; behind a --parent-tree package root)
    import oracle
    import planted
    golden = os.path.join(REPO, "tests", "golden")
    stream = torch.cuda.Stream()
    inputs = [("rx planted", os.path.join(golden, "tables", "rx.npz"),
               lambda: planted.rx_buffer(oracle.xorshift, int(a.gib * (1 << 30)), 19))]   # (rx_1M's generator)
    if mode == "loops" and not a.child:
        inputs.append(("65536 planted Rn6!a..z records", os.path.join(golden, "loops", "tables.npz"),
                       lambda: planted_runs(65536)))
    out = {"reps": a.reps, "classes": "LITERAL | HEX", "runs": []}
    for name, tables, make in inputs:
        host = make()
        n = host.size
        buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        buf[:n] = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        sc = yara_amd.Scanner(yara_amd.Tables.from_npz(tables, strings=True), stream=stream.cuda_stream)
        sc.set_match_classes(yara_amd.MATCH_LITERAL | yara_amd.MATCH_HEX)
        sc.scan_device(buf.data_ptr(), n)
        sc.device_result()

        def stage(on):   # (ms, n_matches, n_rest): the device call alone
            if on is not None:
                getattr(sc, "set_" + mode)(on)
            pm, pr = ctypes.c_void_p(), ctypes.c_void_p()
            nm, nr = ctypes.c_uint64(), ctypes.c_uint64()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check("yr_amd_match_device", _lib.lib().yr_amd_match_device(
                sc._h, 0, ctypes.byref(pm), ctypes.byref(nm), ctypes.byref(pr), ctypes.byref(nr)))
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), nm.value, nr.value

        if a.child:   # the setting is never touched: the same calls on either library
            for _ in range(3):
                stage(None)
            print(json.dumps({"off_ms": med([stage(None)[0] for _ in range(a.reps)])}), flush=True)
            return
        for _ in range(2):   # warm-up: buffers grown, clocks up
            stage(False)
            stage(True)
        off, on = [], []
        for _ in range(a.reps):   # interleaved
            ms, m_off, r_off = stage(False)
            off.append(ms)
            ms, m_on, r_on = stage(True)
            on.append(ms)
        run = {"bytes": n, "input": name, "records": sc.verify_device(0)[1],
               "off": {"matches": m_off, "rest": r_off, "match_device_ms": med(off), "min_max_ms": span(off)},
               "on": {"matches": m_on, "rest": r_on, "match_device_ms": med(on), "min_max_ms": span(on)},
               "added_ms": round(med(on) - med(off), 4), mode[:-1] + "_records": r_off - r_on}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        sc.close()
        del buf
    if mode == "alternations":   # (one input: the file's shape of before)
        out = dict(out, **out.pop("runs")[0])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C,short")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hex", action="store_true",
                    help="the hex class on config C's planted input instead of the sets")
    ap.add_argument("--hex-wide", action="store_true",
                    help="the wave-wide path: the setting off and on, on C's planted input and "
                         "on planted copies of the hexwide fixture's `back` string")
    ap.add_argument("--alternations", action="store_true",
                    help="alternation strings: the setting off and on, on rx's planted input")
    ap.add_argument("--loops", action="store_true",
                    help="loop strings: the setting off and on, on rx's planted input and on "
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
