"""GPU: alternation strings (yr_amd_scanner_set_alternations) against stock libyara's lists on
tests/golden/alternation and the transcription of yr_re_exec that equals them (test_alternation_abi)."""
import gzip
import os

import numpy as np
import pytest

import yara_amd
from conftest import GOLDEN, case_data, golden, tables_npz
from test_alternation_abi import FIX, fixture, settle

pytestmark = pytest.mark.gpu

LIT, HEX = yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX
PATHS = {"alternation": os.path.join(FIX, "tables.npz"), "rx": tables_npz("rx"),
         "hex": tables_npz("hex"), "chain": os.path.join(GOLDEN, "chain", "tables.npz"),
         "both": os.path.join(FIX, "both_tables.npz"), "hex_yarc": tables_npz("hex")}
_CACHE = {}


def tables(name):
    if name not in _CACHE and name == "hex_yarc":         # hex.npz carries no chain links
        with gzip.open(os.path.join(GOLDEN, "yarc", "hex.yarc.gz")) as f:
            _CACHE[name] = (yara_amd.Tables.from_yarc(f.read(), device=0), dict(np.load(PATHS[name])))
    if name not in _CACHE:
        _CACHE[name] = (yara_amd.Tables.from_npz(PATHS[name], device=0, strings=True),
                        dict(np.load(PATHS[name])))
    return _CACHE[name]


def case(name):
    if name == "alternation":
        return fixture()[1]["data"]
    if name in ("chain", "both"):
        return np.load(os.path.join(GOLDEN, *{"chain": ("chain", "case.npz"),
                                              "both": ("alternation", "both_case.npz")}[name]))["data"]
    return case_data(golden()["cases"][name[:3] + "_1M"])


def listed(matches):
    return [tuple(int(m[f]) for f in ("string", "offset", "length", "xor_key")) for m in matches]


def expected(t, z, data, calls, base):
    """(matches, rest) with the setting on: ``base`` (off) + what the transcription settles."""
    alt = t.alternation_strings()
    recs = [(int(r["offset"]), int(r["pool_index"])) for r in calls]
    items, left = settle(z, data, recs, alt)
    assert not alt[base[0]["string"]].any()
    want = sorted(listed(base[0]) + [(s, o, n, 0) for (s, o), n in items.items()])
    settled = alt[z["pool_string"][calls["pool_index"]]]
    settled[left] = False
    gone = {tuple(int(x) for x in r) for r in calls[settled]}
    return want, [r for r in base[1] if tuple(int(x) for x in r) not in gone]


def check(sc, t, z, data, **on):
    base = sc.string_matches(data, hex=True, **on)
    matches, rest = sc.string_matches(data, hex=True, alternations=True, **on)
    want, want_rest = expected(t, z, data, sc.verify_calls(data), base)
    assert listed(matches) == want
    np.testing.assert_array_equal(rest, np.array(want_rest, dtype=rest.dtype))
    return matches, rest, base


@pytest.mark.parametrize("name", ["alternation", "rx", "hex"])
def test_parity(name):
    t, z = tables(name)
    data = case(name)
    matches, rest, base = check(yara_amd.Scanner(t), t, z, data)
    more = t.alternation_strings().any()                  # (hex.yar has no alternative)
    assert (len(matches) > len(base[0]) and len(rest) < len(base[1])) == more
    if name != "alternation":
        return
    # stock libyara's lists, element for element; the 65-byte run alone stays in the rest
    # (wide: `far`, a final hex string of the classes, skips 80 bytes)
    man, a, _ = fixture()
    matches, rest = yara_amd.Scanner(t).string_matches(data, hex=True, wide=True, alternations=True)
    sel = t.match_strings(LIT | HEX) | t.alternation_strings()
    lost = (man["strings"].index("run65"), 896)
    keep = sel[a["match_string"]] & ~((a["match_string"] == lost[0]) & (a["match_offset"] == 896))
    stock = list(zip(a["match_string"][keep], a["match_offset"][keep], a["match_len"][keep],
                     a["match_xor"][keep]))
    assert listed(matches) == [tuple(int(x) for x in m) for m in stock]
    string = z["pool_string"][rest["pool_index"]]
    assert sorted(zip(string[sel[string]], rest["offset"][sel[string]])) == [lost]


def test_off_and_off_again():
    t, z = tables("alternation")
    data, sc = case("alternation"), yara_amd.Scanner(t)
    off = sc.string_matches(data, hex=True)
    on = sc.string_matches(data, hex=True, alternations=True)
    again = sc.string_matches(data, hex=True)
    for x, y in zip(off, again):
        np.testing.assert_array_equal(x, y)
    assert len(on[0]) > len(off[0])
    sc.set_alternations(True)                             # without the hex class: not read
    for x, y in zip(sc.string_matches(data), yara_amd.Scanner(t).string_matches(data)):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.set_alternations(2)
    assert e.value.code == yara_amd.INVALID_ARGUMENT
    bare = yara_amd.Tables.from_npz(PATHS["alternation"], device=0, strings=True, regex=False)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        yara_amd.Scanner(bare).string_matches(data, hex=True, alternations=True)
    assert e.value.code == yara_amd.INVALID_ARGUMENT


@pytest.mark.parametrize("name,on", [("alternation", {"wide": True}), ("hex", {"wide": True}),
                                     ("chain", {"chains": True}), ("hex_yarc", {"chains": True}),
                                     ("chain", {"wide": True, "chains": True}),
                                     ("both", {"chains": True}), ("both", {"wide": True, "chains": True})])
def test_with_wide_and_chains(name, on):
    t, z = tables(name)
    matches, rest, base = check(yara_amd.Scanner(t), t, z, case(name), **on)
    assert set(listed(base[0])) <= set(listed(matches))   # nothing lost
    if "chains" in on:                                    # (hex_1M: string 9's chain, six matches)
        assert t.chain_strings(LIT | HEX).any() and len(base[0]) > len(
            yara_amd.Scanner(t).string_matches(case(name), hex=True, wide="wide" in on)[0])
    if name == "both":
        # chain events and alternation records in one call: stock libyara's lists but for `mixed`,
        # the chain with an alternation part (strings 6, 7), whose calls all stay in the rest
        a = dict(np.load(os.path.join(FIX, "both_case.npz")))
        stock = [tuple(int(x) for x in m) for m in zip(a["match_string"], a["match_offset"],
                                                       a["match_len"], a["match_xor"]) if m[0] != 6]
        assert listed(matches) == stock and {0, 2, 3, 4, 8} == set(matches["string"])
        left = z["pool_string"][rest["pool_index"]]
        assert set(left) == {6, 7} and len(left) == np.isin(
            z["pool_string"][a["verify_idx"]], [6, 7]).sum()
    if name == "alternation":                             # both queues in one call
        far = fixture()[0]["strings"].index("far")
        assert far in matches["string"] and 0 in matches["string"]


def planted(records):
    """`records` copies of the fixture's long_first plant (stock: length 9), 64 bytes apart."""
    buf = np.zeros(records * 64 + 64, np.uint8)
    for r in range(records):
        buf[r * 64 + 8:r * 64 + 17] = (0xAA, 0xBB, 0xCC, 0xDD, 1, 2, 3, 2, 3)
    return buf


# (2100: above the fixed grid's 2048 waves -- the stride loop -- and the queue's first capacity)
@pytest.mark.parametrize("records", [0, 1, 4, 5, 64, 65, 2100])
def test_queue_edges(records):
    t, z = tables("alternation")
    sc = yara_amd.Scanner(t)
    matches, rest, _ = check(sc, t, z, planted(records))
    assert listed(matches) == [(0, r * 64 + 8, 9, 0) for r in range(records)] and len(rest) == 0
    check(sc, t, z, planted(3))                           # the same scanner, the grown queue


def test_window_ends_inside_a_match():
    import torch
    t, z = tables("alternation")
    data, sc = case("alternation"), yara_amd.Scanner(t)
    hi = 134                                              # long_first at 128 runs to 137
    win = torch.zeros(hi + 16, dtype=torch.uint8, device="cuda")
    win[:hi] = torch.from_numpy(data[:hi].copy()).cuda()
    torch.cuda.synchronize()
    sc.scan_window(win.data_ptr(), 0, hi, data.size, 112, hi)
    sc.device_result()
    matches, rest = sc.match_device(hex=True, alternations=True)
    assert 0 not in matches["string"]
    assert ((z["pool_string"][rest["pool_index"]] == 0) & (rest["offset"] == 128)).sum() == 1
