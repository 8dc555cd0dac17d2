"""GPU: the hex class of the match stage (yr_amd_scanner_set_match_classes,
YR_AMD_MATCH_HEX) against stock libyara's match lists, and against a numpy /
Python restatement of _yr_scan_verify_re_match + yr_re_fast_exec in set form."""
import json
import os

import numpy as np
import pytest

import oracle
import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, case_arrays, case_data, golden, tables_npz
from oracle.tables import RefTables
from test_gpu_parity import blocks
from test_hex_match_abi import class_rule, hex_rule

pytestmark = pytest.mark.gpu

LIT, HEX = yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX
CASES = golden()["cases"]
MIB = 1 << 20
WHOLE = [k for k, v in CASES.items()
         if not v["block"] and v["size"] <= MIB and case_arrays(k) is not None]
BLOCKS = [k for k, v in CASES.items()
          if v["block"] and v["size"] <= MIB and case_arrays(k) is not None]
HEXMATCH = os.path.join(GOLDEN, "hexmatch")
RE_SCAN_LIMIT = 4096
_TABLES, _NPZ = {}, {}


def npz_path(name):
    return os.path.join(HEXMATCH, "tables.npz") if name == "hexmatch" else tables_npz(name)


def npz(name):
    if name not in _NPZ:
        _NPZ[name] = dict(np.load(npz_path(name)))
    return _NPZ[name]


def str_tables(name):
    if name not in _TABLES:
        _TABLES[name] = yara_amd.Tables.from_npz(npz_path(name), device=0, strings=True)
    return _TABLES[name]


def assert_fields(got, want, fields=("string", "offset", "length", "xor_key")):
    for f in fields:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


# -- the rule, restated ----------------------------------------------------------
def run_program(code, data, offset, backwards):
    """yr_re_fast_exec (re.c:2150-2423) in set form: the set of bytes_matched
    values at RE_OPCODE_MATCH; None where the device's 64-position window does
    not hold the set or it comes within reach of YR_RE_SCAN_LIMIT."""
    maxb = min(offset if backwards else len(data) - offset, RE_SCAN_LIMIT)
    cur, ip = {0}, 0
    while True:
        op = code[ip]
        if op == 0xAD:                                   # MATCH
            return cur
        live = {b for b in cur if b < maxb}
        if not live:
            return set()
        if op == 0xB5:                                   # REPEAT_ANY_UNGREEDY {min, max}
            mn = code[ip + 1] | code[ip + 2] << 8
            mx = code[ip + 3] | code[ip + 4] << 8
            span = max(live) - min(live) + (mx - mn)
            if span > 63 or min(live) + mn + span >= RE_SCAN_LIMIT:
                return None
            cur = {b + mn for b in live} | {b + j for b in live for j in range(mn + 1, mx + 1)
                                            if b + j < maxb}
            ip += 5
            continue
        a1 = code[ip + 1] if ip + 1 < len(code) else 0
        a2 = code[ip + 2] if ip + 2 < len(code) else 0
        test, size = {
            0xA0: (lambda c: True, 1),                   # ANY
            0xA2: (lambda c: c == a1, 2),                # LITERAL
            0xAE: (lambda c: c != a1, 2),                # NOT_LITERAL
            0xA4: (lambda c: (c & a2) == a1, 3),         # MASKED_LITERAL
            0xAF: (lambda c: (c & a2) != a1, 3),         # MASKED_NOT_LITERAL
        }[op]
        cur = {b + 1 for b in live
               if test(int(data[offset - 1 - b] if backwards else data[offset + b]))}
        if not cur:
            return set()
        ip += size


def measure_record(z, data, k, offset):
    """A final hex string's record -> [(offset, length)], [] for no match, None
    where the device leaves the record to the host."""
    if z["re_kind"][k] == 0 or z["re_fwd_len"][k] == 0:
        return None
    code = z["re_code"]
    fwd = [int(c) for c in code[z["re_fwd_off"][k]:z["re_fwd_off"][k] + z["re_fwd_len"][k]]]
    ends = run_program(fwd, data, offset, False)
    if ends is None:
        return None
    if not ends:
        return []
    f = min(ends)
    if z["re_bwd_len"][k] == 0:
        return [(offset, f)] if f else []
    bwd = [int(c) for c in code[z["re_bwd_off"][k]:z["re_bwd_off"][k] + z["re_bwd_len"][k]]]
    starts = run_program(bwd, data, offset, True)
    if starts is None:
        return None
    return [(offset - b, b + f) for b in sorted(starts)]


def restate(rules, data, recs, classes=LIT | HEX):
    """(matches {string, offset, length, pool_index}, rest, items) of a record
    stream: literal final records are one item each, final hex records what
    measure_record gives; of the items with one (string, offset) the first in
    record order stays; ascending by (string, offset)."""
    z = npz(rules)
    flags = z["str_flags"]
    lit = class_rule(flags, LIT)
    hexs = hex_rule(flags) if classes & HEX else np.zeros(len(flags), bool)
    items, rest = [], []
    for r, rec in enumerate(recs):
        k, off = int(rec["pool_index"]), int(rec["offset"])
        s = int(z["pool_string"][k])
        if lit[s]:
            items.append((s, off, -1, k))
        elif hexs[s]:
            got = measure_record(z, data, k, off)
            if not got:                                  # undecided, or nothing found
                rest.append(r)
            items += [(s, o, n, k) for o, n in got or []]
        else:
            rest.append(r)
    seen, first = set(), []
    for it in items:
        if it[:2] not in seen:
            seen.add(it[:2])
            first.append(it)
    first.sort(key=lambda it: it[:2])
    cols = list(zip(*first)) if first else [[], [], [], []]
    return ({"string": np.array(cols[0], np.uint32), "offset": np.array(cols[1], np.uint64),
             "length": np.array(cols[2], np.int64), "pool_index": np.array(cols[3], np.uint32)},
            recs[np.array(rest, np.int64)], len(items))


def assert_restated(got, want):
    assert_fields(got, want, ("string", "offset", "pool_index"))
    hexm = want["length"] >= 0                           # (literal lengths: the stock goldens')
    np.testing.assert_array_equal(got["length"][hexm], want["length"][hexm])
    assert not got["xor_key"][hexm].any()


def golden_matches(a, rules, classes=LIT | HEX, without=()):
    sel = class_rule(npz(rules)["str_flags"], classes)
    sel[list(without)] = False
    sel = sel[a["match_string"]]
    return {"string": a["match_string"][sel], "offset": a["match_offset"][sel],
            "length": a["match_len"][sel], "xor_key": a["match_xor"][sel]}


# -- stock parity ------------------------------------------------------------------
@pytest.mark.parametrize("case", WHOLE)
def test_stock_parity(case):
    rec = CASES[case]
    data = case_data(rec)
    z = npz(rec["rules"])
    sc = yara_amd.Scanner(str_tables(rec["rules"]))
    matches, rest = sc.string_matches(data, hex=True)
    want = golden_matches(case_arrays(case), rec["rules"])
    assert_fields(matches, want)
    if case == "hex_1M":
        hexm = hex_rule(z["str_flags"])[want["string"]]
        assert hexm.sum() == 53
        per_string = [len(set(want["length"][want["string"] == s])) for s in set(want["string"])]
        assert max(per_string) == 5
    # the rest: the calls of the other strings, unchanged -- none of the classes'
    calls = sc.verify_calls(data)
    other = ~class_rule(z["str_flags"], LIT | HEX)[z["pool_string"][calls["pool_index"]]]
    assert_fields(rest, calls[other], ("offset", "pool_index", "candidate"))
    # and the restatement agrees with stock libyara
    assert_restated(matches, restate(rec["rules"], data, calls)[0])


def test_goldens_with_weight():
    z = {c: hex_rule(npz(CASES[c]["rules"])["str_flags"])[case_arrays(c)["match_string"]].sum()
         for c in ("hex_1M", "fuzz0_256K", "fuzz5_256K", "fuzz8_256K")}
    assert all(v > 0 for v in z.values()), z


@pytest.mark.parametrize("case", ["hex_1M", "lit_1M"])
def test_default_unchanged(case):
    rec = CASES[case]
    data = case_data(rec)
    t = str_tables(rec["rules"])
    fresh = yara_amd.Scanner(t).string_matches(data)
    sc = yara_amd.Scanner(t)
    sc.set_match_classes(LIT | HEX)
    with_hex = sc.string_matches(data)
    sc.set_match_classes(LIT)
    back = sc.string_matches(data)
    for a, b in zip(fresh, back):
        np.testing.assert_array_equal(a, b)
    # hex=True is the classes for one call
    once = sc.string_matches(data, hex=True)
    for a, b in zip(with_hex, once):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(fresh, sc.string_matches(data)):
        np.testing.assert_array_equal(a, b)
    if case == "hex_1M":
        assert len(with_hex[0]) == len(fresh[0]) + 53 and len(with_hex[1]) < len(fresh[1])


@pytest.mark.parametrize("case", BLOCKS)
def test_overlapping_blocks(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = yara_amd.Scanner(str_tables(rec["rules"]))
    per_block = []
    for b, n in blocks(data.size, rec["block"], rec["overlap"]):
        per_block.append((b, sc.string_matches(data[b:b + n], data_base=b, hex=True)[0]))
    assert_fields(yara_amd.merge_matches(per_block),
                  golden_matches(case_arrays(case), rec["rules"]))


# -- the fixture of shapes -----------------------------------------------------------
TWO_BACK, SHORTEST, SAME_START, WIDE = 0, 1, 2, 3


def fixture():
    with open(os.path.join(HEXMATCH, "manifest.json")) as f:
        man = json.load(f)
    a = dict(np.load(os.path.join(HEXMATCH, "case.npz")))
    assert man["strings"][:4] == ["two_back", "shortest", "same_start", "wide"]
    assert a["data"].size == man["size"] <= 64 << 10
    return man, a


def test_fixture_shapes():
    man, a = fixture()
    data, z = a["data"], npz("hexmatch")
    n = data.size
    sc = yara_amd.Scanner(str_tables("hexmatch"))
    matches, rest = sc.string_matches(data, hex=True)
    # stock libyara's lists, but for the wide jump's string
    assert_fields(matches, golden_matches(a, "hexmatch", without=[WIDE]))
    calls = sc.verify_calls(data)
    string = z["pool_string"][calls["pool_index"]]
    keep = ~class_rule(z["str_flags"], LIT | HEX)[string] | (string == WIDE)
    assert_fields(rest, calls[keep], ("offset", "pool_index", "candidate"))
    in_class = class_rule(z["str_flags"], LIT | HEX)[z["pool_string"][rest["pool_index"]]]
    assert set(z["pool_string"][rest["pool_index"]][in_class]) == {WIDE}
    assert (a["match_string"] == WIDE).sum() == 3 and (string == WIDE).sum() >= 3
    want, want_rest, items = restate("hexmatch", data, calls)
    assert_restated(matches, want)
    assert_fields(rest, want_rest, ("offset", "pool_index", "candidate"))
    # the shapes are there: one call with at least 4 offsets ...
    per_call = {}
    for r in calls[string == TWO_BACK]:
        per_call[int(r["offset"])] = measure_record(z, data, int(r["pool_index"]), int(r["offset"]))
    assert max(len(v) for v in per_call.values()) >= 4
    # ... a backward run cut at the buffer's start ...
    k_two = int(calls[string == TWO_BACK][0]["pool_index"])
    assert (0, 7) in per_call[min(per_call)] and min(per_call) < 2 * 3 + 2
    assert z["re_bwd_len"][k_two] > 1
    # ... the shortest of several continuations ...
    m = matches[matches["string"] == SHORTEST]
    at = int(m["offset"][0])
    assert bytes(data[at + 4:at + 10]) == bytes.fromhex("d5d6d5d6d5d6") and m["length"][0] == 6
    # ... a forward run that ends at the last byte ...
    assert int(m["offset"][-1]) + int(m["length"][-1]) == n
    # ... and two calls with one (string, offset): the first one's length
    starts = [o for r in calls[string == SAME_START]
              for o, _ in measure_record(z, data, int(r["pool_index"]), int(r["offset"]))]
    assert len(starts) > len(set(starts)) and items > len(matches)
    first = matches[(matches["string"] == SAME_START)][0]
    assert first["length"] == 5


# -- wave and workspace edges ----------------------------------------------------------
EDGE_ITEMS = [0, 1, 63, 64, 65, 256, 257, 20000]
UNIT = 32
FOUR = bytes.fromhex("c1c1c1c1c2c2c2c2c3c4c5c6c7")    # $two_back: one record, 4 items
ONE = bytes.fromhex("d1d2d3d4d5d6")                    # $shortest: one record, one item
TWICE = bytes.fromhex("e1e2e3e4e5e2e3e4e5")            # $same_start: two records, one offset


def edge_buffer(items):
    """Planted copies, UNIT bytes apart in zeros, that make `items` items."""
    twice = 100 if items >= 1000 else 0
    four, one = divmod(items - 2 * twice, 4)
    units = [FOUR] * four + [TWICE] * twice + [ONE] * one
    buf = np.zeros(max(len(units), 1) * UNIT + 5, np.uint8)   # (no multiple of anything)
    for u, b in enumerate(units):
        # spread the kinds: the records of one wave differ in their item counts
        at = (u * 7919 % len(units)) * UNIT + 3
        buf[at:at + len(b)] = np.frombuffer(b, np.uint8)
    return buf


def cpu_records(rules, data):
    z = npz(rules)
    tab = RefTables(z["T"], z["M"], z["pool_next"], z["pool_string"], z["pool_backtrack"])
    pos, idx = oracle.walk_verify(tab, data)
    keep = oracle.literal_effect(z, pos, idx, data).astype(bool)
    recs = np.zeros(int(keep.sum()), dtype=_lib.VERIFY_REC_DTYPE)
    recs["offset"] = (pos - z["pool_backtrack"][idx])[keep]
    recs["pool_index"] = idx[keep]
    return recs


@pytest.mark.parametrize("items", EDGE_ITEMS)
def test_wave_and_workspace_edges(items):
    data = edge_buffer(items)
    recs = cpu_records("hexmatch", data)
    want, want_rest, n_items = restate("hexmatch", data, recs)
    assert n_items == items and len(want_rest) == 0
    if items >= 1000:
        assert len(want["string"]) == items - 100
    sc = yara_amd.Scanner(str_tables("hexmatch"))
    matches, rest = sc.string_matches(data, hex=True)
    assert_restated(matches, want)
    assert len(rest) == 0
    # and through the device calls, on the same scanner again (a workspace that grew)
    import torch
    d = torch.zeros(max(data.size, 16), dtype=torch.uint8, device="cuda")
    d[:data.size] = torch.from_numpy(data.copy()).cuda()
    sc.scan_device(d.data_ptr(), data.size)
    sc.device_result()
    m2, r2 = sc.match_device(hex=True)
    np.testing.assert_array_equal(m2, matches)
    assert len(r2) == 0


# -- windows ------------------------------------------------------------------------------
def window_matches(sc, torch, data, lo, hi, begin, end):
    win = torch.zeros(max(hi - lo, 16), dtype=torch.uint8, device="cuda")
    win[:hi - lo] = torch.from_numpy(data[lo:hi].copy()).cuda()
    torch.cuda.synchronize()
    sc.scan_window(win.data_ptr(), lo, hi, data.size, begin, end)
    sc.device_result()
    return sc.match_device(hex=True)


def test_windows():
    import torch
    from yara_amd import dist as ydist
    rec = CASES["hex_1M"]
    data = case_data(rec)
    n = data.size
    t = str_tables("hex")
    z = npz("hex")
    cls = class_rule(z["str_flags"], LIT | HEX)
    sc = yara_amd.Scanner(t)
    whole, _ = sc.string_matches(data, hex=True)
    assert len(whole) >= 53
    before, after = ydist.tables_halos(t)
    cut = 500000 // 16 * 16
    parts = []
    for begin, end in ((0, cut), (cut, n)):
        lo, hi = ydist.shard_window(n, begin, end, before, after)
        assert (lo, hi) != (0, n)
        m, rest = window_matches(sc, torch, data, lo, hi, begin, end)
        assert not cls[z["pool_string"][rest["pool_index"]]].any()
        parts.append(m)
    assert len(parts[0]) and len(parts[1])
    both = yara_amd.merge_matches([(0, parts[0]), (0, parts[1])])
    assert_fields(both, whole, ("string", "offset", "length", "xor_key", "pool_index"))

    # a window that ends inside a hex match: a byte the forward run may read is
    # not held, so the record is no match yet -- it stays with the host
    calls = sc.verify_calls(data)
    bt = z["pool_backtrack"].astype(np.int64)
    pick = call = None
    for cand in whole[(whole["length"] >= 8) & (whole["offset"] > 8192)]:
        o, length, k = int(cand["offset"]), int(cand["length"]), int(cand["pool_index"])
        mine = calls[(calls["pool_index"] == k) & (calls["offset"] >= o) &
                     (calls["offset"] < o + length)]
        if len(mine) == 1 and int(mine[0]["offset"]) + bt[k] + 1 < o + length:
            pick, call = cand, mine[0]
            break
    assert pick is not None
    o, length, ro = int(pick["offset"]), int(pick["length"]), int(call["offset"])
    hi = o + length - 1                     # the match's last byte is not held
    lo = max(0, o - before - 64) // 16 * 16
    begin = (o - 16) // 16 * 16
    assert begin < ro + bt[pick["pool_index"]] <= hi
    m, rest = window_matches(sc, torch, data, lo, hi, begin, hi)
    here = (rest["offset"] == ro) & (rest["pool_index"] == pick["pool_index"])
    assert here.sum() == 1
    assert not ((m["string"] == pick["string"]) & (m["offset"] == o)).any()
    # the scanner is still good for the whole block
    assert_fields(sc.string_matches(data, hex=True)[0], whole)


# -- misuse -----------------------------------------------------------------------------------
def test_misuse():
    import torch
    INV = yara_amd.INVALID_ARGUMENT
    rec = CASES["hex_1M"]
    data = case_data(rec)[:1 << 18]
    sc = yara_amd.Scanner(str_tables("hex"))
    for classes in (0, HEX, 4, LIT | 4, LIT | HEX | 8):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.set_match_classes(classes)
        assert e.value.code == INV
    want, want_rest = sc.string_matches(data, hex=True)
    assert len(want) > 5
    # tables without the strings' programs
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(tables_npz("hex"), device=0, strings=True,
                                                     regex=False))
    lit_only = bare.string_matches(data)
    bare.set_match_classes(LIT | HEX)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.string_matches(data)
    assert e.value.code == INV
    d = torch.from_numpy(data.copy()).cuda()
    bare.scan_device(d.data_ptr(), data.size)
    bare.device_result()
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.match_device()
    assert e.value.code == INV
    bare.set_match_classes(LIT)
    np.testing.assert_array_equal(bare.match_device()[0], lit_only[0])
    # a batch: the setting is ignored (literal-only), and match_device refuses a batch scan
    sc.set_match_classes(LIT | HEX)
    bufs = [data[:70000], data[70000:150001]]
    got = sc.batch_string_matches(bufs)
    ref = yara_amd.Scanner(str_tables("hex")).batch_string_matches(bufs)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.match_device()
    assert e.value.code == INV
    np.testing.assert_array_equal(sc.string_matches(data)[0], want)
    # profiling tables (their own: the setting is the tables')
    tp = yara_amd.Tables.from_npz(tables_npz("hex"), device=0, strings=True)
    tp.set_profiling(True)
    sp = yara_amd.Scanner(tp)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sp.string_matches(data, hex=True)
    assert e.value.code == INV
    tp.set_profiling(False)
    np.testing.assert_array_equal(sp.string_matches(data, hex=True)[0], want)
    # a block declared above YR_AMD_MATCH_MAX_BLOCK
    limit = _lib.MATCH_MAX_BLOCK
    sc.scan_window(d.data_ptr(), limit, limit + data.size, limit + (2 << 20), limit + 16,
                   limit + data.size)
    sc.device_result()
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.match_device(hex=True)
    assert e.value.code == INV
    np.testing.assert_array_equal(sc.string_matches(data)[1], want_rest)
