"""GPU: the match stage (yr_amd_match_device) against stock libyara's match
lists.  The golden match_* arrays were written by the reference
(oracle/refdump.c dump_all_matches), ordered by string, then offset."""
import gzip
import os

import numpy as np
import pytest

import oracle
import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, case_arrays, case_data, golden, ref_tables, tables_npz
from test_gpu_parity import blocks
from test_match_abi import final_rule

pytestmark = pytest.mark.gpu

CASES = golden()["cases"]
MIB = 1 << 20
WHOLE = [k for k, v in CASES.items()
         if not v["block"] and v["size"] <= MIB and case_arrays(k) is not None]
BLOCKS = [k for k, v in CASES.items()
          if v["block"] and v["size"] <= MIB and case_arrays(k) is not None]
_TABLES, _NPZ = {}, {}


def npz(name):
    if name not in _NPZ:
        _NPZ[name] = dict(np.load(tables_npz(name)))
    return _NPZ[name]


def str_tables(name):
    if name not in _TABLES:
        _TABLES[name] = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    return _TABLES[name]


def test_case_lists():
    assert set(WHOLE) == {"lit_1M", "short_1M", "hex_1M", "rx_1M", "root_4K", "short_3",
                          "A_sample", "C_empty"} | {"fuzz%d_256K" % k for k in range(12)}
    assert set(BLOCKS) == {"lit_1M_blocks", "short_1M_blocks", "hex_1M_blocks", "rx_1M_blocks",
                           "fuzz0_256K_blocks", "fuzz1_256K_blocks", "fuzz2_256K_blocks"}


def golden_matches(case, rules):
    """The stock match lists restricted to the final strings."""
    a = case_arrays(case)
    sel = final_rule(npz(rules)["str_flags"])[a["match_string"]]
    return {"string": a["match_string"][sel], "offset": a["match_offset"][sel],
            "length": a["match_len"][sel], "xor_key": a["match_xor"][sel]}


def assert_fields(got, want, fields=("string", "offset", "length", "xor_key")):
    for f in fields:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def restate(rules, recs):
    """The rule in numpy: (matches' string, offset, pool_index; rest) of a
    record stream -- the final strings' records, the first of every (string,
    offset) in record order, ascending by (string, offset)."""
    z = npz(rules)
    string = z["pool_string"][recs["pool_index"]]
    fin = final_rule(z["str_flags"])[string] if recs.size else np.zeros(0, bool)
    rest = recs[~fin]
    m, s = recs[fin], string[fin]
    key = s.astype(np.uint64) << np.uint64(32) | m["offset"]
    _, first = np.unique(key, return_index=True)   # first occurrence, ascending by key
    return {"string": s[first], "offset": m["offset"][first],
            "pool_index": m["pool_index"][first]}, rest


@pytest.mark.parametrize("case", WHOLE)
def test_stock_parity(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = yara_amd.Scanner(str_tables(rec["rules"]))
    matches, rest = sc.string_matches(data)
    assert_fields(matches, golden_matches(case, rec["rules"]))
    calls = sc.verify_calls(data)
    _, want_rest = restate(rec["rules"], calls)
    assert_fields(rest, want_rest, ("offset", "pool_index", "candidate"))
    assert len(matches) + len(rest) <= len(calls)


@pytest.mark.parametrize("case", BLOCKS)
def test_overlapping_blocks(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = yara_amd.Scanner(str_tables(rec["rules"]))
    per_block = []
    for b, n in blocks(data.size, rec["block"], rec["overlap"]):
        per_block.append((b, sc.string_matches(data[b:b + n], data_base=b)[0]))
    assert_fields(yara_amd.merge_matches(per_block), golden_matches(case, rec["rules"]))


# -- wave and group edges ------------------------------------------------------
EDGE_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]
_EDGE = {}


def record_count(z, tab, data):
    pos, idx = oracle.walk_verify(tab, data)
    return int(oracle.literal_effect(z, pos, idx, data).sum())


def edge_prefixes():
    """Prefix lengths of short_1M's data whose record counts are EDGE_COUNTS and
    about 20,000, found on the CPU (the oracle's walk and keep rule)."""
    if not _EDGE:
        data = case_data(CASES["short_1M"])
        z, tab = npz("short"), ref_tables("short")
        pos, idx = oracle.walk_verify(tab, data)
        cum = np.cumsum(oracle.literal_effect(z, pos, idx, data))
        for want in EDGE_COUNTS:
            # a prefix ends calls that the whole block keeps, so its count can
            # only be smaller: walk on from the first length that could do
            n = int(pos[np.searchsorted(cum, want)]) if want else 0
            while record_count(z, tab, data[:n]) < want:
                n += 1
            assert record_count(z, tab, data[:n]) == want, want
            _EDGE[want] = n
        n = int(pos[np.searchsorted(cum, 20000)])
        _EDGE[record_count(z, tab, data[:n])] = n
        _EDGE["data"] = data
    return _EDGE


def test_edge_prefixes_exist():
    e = edge_prefixes()
    counts = sorted(k for k in e if k != "data")
    assert counts[:-1] == EDGE_COUNTS and 19000 <= counts[-1] <= 20000


@pytest.mark.parametrize("which", range(len(EDGE_COUNTS) + 1))
def test_wave_and_group_edges(which):
    e = edge_prefixes()
    count = sorted(k for k in e if k != "data")[which]
    data = e["data"][:e[count]]
    sc = yara_amd.Scanner(str_tables("short"))
    calls = sc.verify_calls(data)
    assert len(calls) == count
    matches, rest = sc.string_matches(data)
    want, want_rest = restate("short", calls)
    assert_fields(matches, want, ("string", "offset", "pool_index"))
    assert_fields(rest, want_rest, ("offset", "pool_index", "candidate"))
    # and through the device calls, on the same scanner again
    import torch
    d = torch.zeros(max(data.size, 16), dtype=torch.uint8, device="cuda")
    d[:data.size] = torch.from_numpy(data.copy()).cuda()
    sc.scan_device(d.data_ptr(), data.size)
    sc.device_result()
    m2, r2 = sc.match_device()
    assert_fields(m2, matches, ("string", "offset", "length", "xor_key", "pool_index"))
    assert_fields(r2, rest, ("offset", "pool_index"))


# -- windows -------------------------------------------------------------------
def window_matches(sc, torch, data, lo, hi, begin, end):
    win = torch.zeros(max(hi - lo, 16), dtype=torch.uint8, device="cuda")
    win[:hi - lo] = torch.from_numpy(data[lo:hi].copy()).cuda()
    torch.cuda.synchronize()
    sc.scan_window(win.data_ptr(), lo, hi, data.size, begin, end)
    sc.device_result()
    return sc.match_device()


def test_windows():
    import torch
    from yara_amd import dist as ydist
    rec = CASES["lit_1M"]
    data = case_data(rec)
    n = data.size
    t = str_tables("lit")
    z = npz("lit")
    fin = final_rule(z["str_flags"])
    sc = yara_amd.Scanner(t)
    whole, _ = sc.string_matches(data)
    assert len(whole) > 100
    before, after = ydist.tables_halos(t)
    cut = 500000 // 16 * 16
    parts = []
    for begin, end in ((0, cut), (cut, n)):
        lo, hi = ydist.shard_window(n, begin, end, before, after)
        assert (lo, hi) != (0, n)
        m, rest = window_matches(sc, torch, data, lo, hi, begin, end)
        assert not fin[z["pool_string"][rest["pool_index"]]].any()
        parts.append(m)
    assert len(parts[0]) and len(parts[1])
    both = yara_amd.merge_matches([(0, parts[0]), (0, parts[1])])
    assert_fields(both, whole, ("string", "offset", "length", "xor_key", "pool_index"))

    # a window that ends inside a match: the call is kept undecided by the
    # pre-verification, so it is no match yet -- it stays with the host
    bt = z["pool_backtrack"][whole["pool_index"]].astype(np.int64)
    inside = np.flatnonzero((whole["length"] >= 8) & (bt + 1 < whole["length"]) &
                            (whole["offset"] > 8192))
    pick = whole[inside[len(inside) // 2]]
    o, length = int(pick["offset"]), int(pick["length"])
    hi = o + length - 1                     # the match's last byte is not held
    lo = max(0, o - before - 64) // 16 * 16
    begin = (o - 16) // 16 * 16
    assert begin < o + int(z["pool_backtrack"][pick["pool_index"]]) <= hi
    m, rest = window_matches(sc, torch, data, lo, hi, begin, hi)
    here = (rest["offset"] == o) & (rest["pool_index"] == pick["pool_index"])
    assert here.sum() == 1
    assert not ((m["string"] == pick["string"]) & (m["offset"] == o)).any()
    # the scanner is still good for the whole block
    assert_fields(sc.string_matches(data)[0], whole)


# -- misuse --------------------------------------------------------------------
def test_misuse():
    import torch
    INV = yara_amd.INVALID_ARGUMENT
    rec = CASES["lit_1M"]
    data = case_data(rec)[:1 << 18]
    sc = yara_amd.Scanner(str_tables("lit"))
    with pytest.raises(yara_amd.YaraAmdError) as e:   # before any scan
        sc.match_device()
    assert e.value.code == INV
    want, _ = sc.string_matches(data)
    assert len(want) > 10
    sc.batch_candidates([data[:70000], data[70000:150001]])   # a completed batch scan
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.match_device()
    assert e.value.code == INV
    d = torch.from_numpy(data.copy()).cuda()
    sc.scan_device(d.data_ptr(), data.size)
    with pytest.raises(yara_amd.YaraAmdError) as e:   # the scan's result not collected
        sc.match_device()
    assert e.value.code == INV
    sc.device_result()
    got, _ = sc.match_device()
    assert_fields(got, want, ("string", "offset", "length", "xor_key", "pool_index"))
    # tables without strings; profiling tables (their own: the setting is the tables')
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(tables_npz("lit"), device=0))
    bare.candidates(data)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.match_device()
    assert e.value.code == INV
    tp = yara_amd.Tables.from_npz(tables_npz("lit"), device=0, strings=True)
    tp.set_profiling(True)
    sp = yara_amd.Scanner(tp)
    sp.scan_device(d.data_ptr(), data.size)
    sp.device_result()
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sp.match_device()
    assert e.value.code == INV
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sp.string_matches(data)
    assert e.value.code == INV
    tp.set_profiling(False)
    assert_fields(sp.string_matches(data)[0], want)


def test_block_size_limit():
    """Offsets are positions of the block, a window's too, and the stage keys
    them in 32 bits: a block of more than YR_AMD_MATCH_MAX_BLOCK = 2^32 bytes
    is refused, whatever the window's size and although the pre-verification
    takes it; a block of exactly 2^32 bytes works up to its last byte."""
    import torch
    rec = CASES["lit_1M"]
    data = case_data(rec)
    n = data.size
    limit = _lib.MATCH_MAX_BLOCK
    assert limit == 1 << 32
    sc = yara_amd.Scanner(str_tables("lit"))
    whole, _ = sc.string_matches(data)
    win = torch.from_numpy(data.copy()).cuda()
    torch.cuda.synchronize()
    # the block's last MiB, the block exactly at the limit: offsets up to 2^32 - 1
    lo = limit - n
    sc.scan_window(win.data_ptr(), lo, limit, limit, lo + 16, limit)   # (4 warm-up bytes held)
    sc.device_result()
    m, rest = sc.match_device()
    assert int(m["offset"].max()) > limit - n // 2 and int(m["offset"].min()) >= lo
    assert np.all(np.diff(m["string"].astype(np.int64) << 33 | m["offset"].astype(np.int64)) > 0)
    have = {(int(r["string"]), int(r["offset"]), int(r["length"]), int(r["xor_key"])) for r in whole}
    got = {(int(r["string"]), int(r["offset"]) - lo, int(r["length"]), int(r["xor_key"])) for r in m}
    # a call within YR_RE_SCAN_LIMIT of the window's start stays undecided (the
    # rest); every later one is decided as in the whole block
    # (not the strings at a FIXED_OFFSET, 0x8000: their place is another one here)
    fixed = (npz("lit")["str_flags"] & 0x8000) != 0
    sure = {x for x in have if x[1] >= 4096 and not fixed[x[0]]}
    assert sure <= got <= have and len(sure) > 100
    # the same window in a block one byte larger, and well inside a larger block
    for size, at in ((limit + 1, lo), (limit + (2 << 20), limit)):
        sc.scan_window(win.data_ptr(), at, at + n, size, at + 16, at + n)
        _, cnt, _ = sc.device_result()
        assert cnt > 0
        assert sc.verify_device(0)[1] > 0          # the pre-verification takes the block
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.match_device()
        assert e.value.code == yara_amd.INVALID_ARGUMENT
    # the scanner is still good
    assert_fields(sc.string_matches(data)[0], whole)


# -- tables from a compiled rules file -----------------------------------------
def test_yarc_tables_give_the_same_matches():
    with gzip.open(os.path.join(GOLDEN, "yarc", "C.yarc.gz")) as f:
        ty = yara_amd.Tables.from_yarc(f.read(), device=0)
    data = case_data(CASES["C_planted16M"])[:MIB]
    a, ra = yara_amd.Scanner(ty).string_matches(data)
    b, rb = yara_amd.Scanner(str_tables("C")).string_matches(data)
    assert len(b) > 100
    assert a.dtype == np.dtype(_lib.MATCH_REC_DTYPE)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ra, rb)
    np.testing.assert_array_equal(ty.final_strings(), str_tables("C").final_strings())
