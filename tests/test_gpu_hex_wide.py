"""GPU: the wave-wide path of the hex class (yr_amd_scanner_set_hex_wide) against stock
libyara's match lists (tests/golden/hexwide) and a set-form restatement that equals them there.
Stock libyara on the two-jump forward plants (`order`, 3072; `order_narrow`, 3328): length 11
where the smallest bytes_matched at MATCH is 10 -- its list's first element, not the minimum.
With the wide path on both records stay in the rest."""
import json
import os

import numpy as np
import pytest

import yara_amd
from conftest import GOLDEN, case_data, golden, tables_npz
from test_hex_match_abi import class_rule

pytestmark = pytest.mark.gpu

LIT, HEX = yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX
FIELDS = ("string", "offset", "length", "xor_key")
PATHS = {"hexwide": os.path.join(GOLDEN, "hexwide", "tables.npz"),
         "hexmatch": os.path.join(GOLDEN, "hexmatch", "tables.npz"), "hex": tables_npz("hex")}
_CACHE = {}


def tables(name):
    if name not in _CACHE:
        _CACHE[name] = (yara_amd.Tables.from_npz(PATHS[name], device=0, strings=True),
                        dict(np.load(PATHS[name])))
    return _CACHE[name]


def fixture(name="hexwide"):
    with open(os.path.join(GOLDEN, name, "manifest.json")) as f:
        man = json.load(f)
    return man, dict(np.load(os.path.join(GOLDEN, name, "case.npz")))


def equal(got, want, fields=FIELDS):
    for f in fields:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


# -- the rule in set form: bit b of S is bytes_matched = b ---------------------------
def wide_run(code, data, offset, back):
    """The set at MATCH; None: a forward jump run from several positions."""
    maxb = min(offset if back else len(data) - offset, 4096)
    S, ip = 1, 0
    while code[ip] != 0xAD:
        live = S & ((1 << maxb) - 1)
        if not live:
            return 0
        op, a1, a2 = code[ip], code[ip + 1], code[ip + 2]
        if op == 0xB5:
            mn, mx = a1 | a2 << 8, code[ip + 3] | code[ip + 4] << 8
            if not back and mx > mn and live & (live - 1):
                return None
            S = 0
            for d in range(mn, mx + 1):                   # (b + mn at or past maxb dies next)
                S |= live << d & ((1 << maxb) - 1)
            ip += 5
            continue
        test, size = {0xA0: (lambda c: True, 1), 0xA2: (lambda c: c == a1, 2),
                      0xAE: (lambda c: c != a1, 2), 0xA4: (lambda c: (c & a2) == a1, 3),
                      0xAF: (lambda c: (c & a2) != a1, 3)}[op]
        S = sum(1 << (b + 1) for b in range(maxb) if live >> b & 1 and
                test(int(data[offset - 1 - b] if back else data[offset + b])))
        ip += size
    return S


def expected(z, data, recs):
    """(hex strings' matches, rest record indexes) of a record stream with the wide
    path on; a final literal string's record is a match (stock's lists say which)."""
    cls, code = class_rule(z["str_flags"], LIT | HEX), [int(c) for c in z["re_code"]]
    lit = class_rule(z["str_flags"], LIT)
    items, rest = {}, []
    for r, rec in enumerate(recs):
        k, off = int(rec["pool_index"]), int(rec["offset"])
        s = int(z["pool_string"][k])
        if not cls[s] or lit[s]:
            rest += [] if lit[s] else [r]
            continue
        f = wide_run(code[z["re_fwd_off"][k]:], data, off, False)
        b = wide_run(code[z["re_bwd_off"][k]:], data, off, True) if z["re_bwd_len"][k] else 1
        if not f or not b:
            rest.append(r)
            continue
        F = (f & -f).bit_length() - 1
        for B in range(b.bit_length()):
            if b >> B & 1:
                items.setdefault((s, off - B), B + F)
    keys = sorted(items)
    return ({"string": np.array([k[0] for k in keys], np.uint32),
             "offset": np.array([k[1] for k in keys], np.uint64),
             "length": np.array([items[k] for k in keys], np.uint32),
             "xor_key": np.zeros(len(keys), np.uint32)}, rest)


def stock(a, z, drop=()):
    sel = class_rule(z["str_flags"], LIT | HEX)[a["match_string"]]
    for s, o in drop:
        sel &= ~((a["match_string"] == s) & (a["match_offset"] == o))
    return {"string": a["match_string"][sel], "offset": a["match_offset"][sel],
            "length": a["match_len"][sel], "xor_key": a["match_xor"][sel]}


# -- the fixture -----------------------------------------------------------------------
def test_fixture_wide_on():
    man, a = fixture()
    t, z = tables("hexwide")
    data, names = a["data"], man["strings"]
    sc = yara_amd.Scanner(t)
    matches, rest = sc.string_matches(data, hex=True, wide=True)
    calls = sc.verify_calls(data)
    # the two plants whose forward jump runs from two positions: stock's first list element
    order = [(names.index("order"), 3072), (names.index("order_narrow"), 3328)]
    equal(matches, stock(a, z, drop=order))
    want, want_rest = expected(z, data, calls)
    equal(matches[~class_rule(z["str_flags"], LIT)[matches["string"]]], want)
    equal(rest, calls[want_rest], ("offset", "pool_index", "candidate"))
    string = z["pool_string"][rest["pool_index"]]
    in_class = class_rule(z["str_flags"], LIT | HEX)[string]
    assert in_class.sum() == man["order_excluded"] == len(order)
    assert sorted(zip(string[in_class], rest["offset"][in_class])) == order
    # the value YR_RE_SCAN_LIMIT itself is a bytes_matched of the reference's
    assert 4096 + 4 in matches["length"][matches["string"] == names.index("limit")]


def test_fixture_wide_off():
    man, a = fixture()
    t, z = tables("hexwide")
    data = a["data"]
    sc = yara_amd.Scanner(t)
    off = sc.string_matches(data, hex=True)
    on = sc.string_matches(data, hex=True, wide=True)
    again = sc.string_matches(data, hex=True)             # the setting was for one call
    for x, y in zip(off, again):
        np.testing.assert_array_equal(x, y)
    assert len(on[0]) > len(off[0]) and len(on[1]) < len(off[1])
    narrow = {man["strings"].index(s) for s in ("order_narrow", "text")}
    assert set(off[0]["string"]) == narrow
    assert {0, 2, 3, 5, 8} <= set(z["pool_string"][off[1]["pool_index"]])   # fwd, back, ... limit


@pytest.mark.parametrize("name", ["hexmatch", "hex_1M"])
def test_existing_results_stay(name):
    if name == "hexmatch":
        (t, z), data = tables("hexmatch"), fixture("hexmatch")[1]["data"]
    else:
        (t, z), data = tables("hex"), case_data(golden()["cases"]["hex_1M"])
    sc = yara_amd.Scanner(t)
    m0, r0 = sc.string_matches(data, hex=True)
    m1, r1 = sc.string_matches(data, hex=True, wide=True)
    have = {tuple(int(x) for x in m) for m in m1}
    assert all(tuple(int(x) for x in m) in have for m in m0)
    today = {tuple(int(x) for x in r) for r in r0}
    assert all(tuple(int(x) for x in r) in today for r in r1) and len(r1) <= len(r0)
    if name == "hexmatch":                                # its `wide` string: stock's three
        assert 3 not in m0["string"] and (z["pool_string"][r0["pool_index"]] == 3).sum() >= 3
        equal(m1, stock(fixture("hexmatch")[1], z))


def test_windows():
    import torch
    from yara_amd import dist as ydist
    man, a = fixture()
    t, z = tables("hexwide")
    data, n = a["data"], a["data"].size
    sc = yara_amd.Scanner(t)
    whole, _ = sc.string_matches(data, hex=True, wide=True)
    before, after = ydist.tables_halos(t)

    def window(lo, hi, begin, end):
        win = torch.zeros(max(hi - lo, 16), dtype=torch.uint8, device="cuda")
        win[:hi - lo] = torch.from_numpy(data[lo:hi].copy()).cuda()
        torch.cuda.synchronize()
        sc.scan_window(win.data_ptr(), lo, hi, n, begin, end)
        sc.device_result()
        return sc.match_device(hex=True, wide=True)

    cut, parts = 20000, []
    for begin, end in ((0, cut), (cut, n)):
        lo, hi = ydist.shard_window(n, begin, end, before, after)
        assert (lo, hi) != (0, n)
        parts.append(window(lo, hi, begin, end)[0])
    equal(yara_amd.merge_matches([(0, parts[0]), (0, parts[1])]), whole,
          FIELDS + ("pool_index",))
    # a window that ends inside the reach of the `fwd` record at 896 (continuation at 1000)
    m, rest = window(0, 990, 880, 990)
    fwd = man["strings"].index("fwd")
    assert fwd not in m["string"]
    assert ((z["pool_string"][rest["pool_index"]] == fwd) & (rest["offset"] == 896)).sum() == 1


# -- item counts and the queue's stride --------------------------------------------------
def counted(items, records):
    """`records` copies of a `two` (items > 101) or `back` plant of `items` matches
    each, 512 bytes apart, a narrow record (`order_narrow`) after each."""
    buf = np.zeros(records * 512 + 300, np.uint8)
    for r in range(records):
        at = r * 512 + 256                                # the atom
        if items > 101:                                   # E6 at 0 and 100, E5 elsewhere to 201
            depth = [d for d in range(1, 202) if d != 100][:items]
            buf[[at - 1 - d for d in depth]] = 0xE5
            buf[[at - 1, at - 101]] = 0xE6
            buf[at:at + 4] = (0xE1, 0xE2, 0xE3, 0xE4)
        else:
            buf[at - items:at] = 0xB5
            buf[at:at + 4] = (0xB1, 0xB2, 0xB3, 0xB4)
        buf[at + 8:at + 15] = (0x71, 0x72, 0x73, 0x74, 0x75, 0, 0)
        buf[at + 15] = 0x76
    return buf


@pytest.mark.parametrize("items,records", [(1, 1), (64, 1), (65, 1), (200, 1), (3, 64), (3, 65)])
def test_item_counts(items, records):
    t, z = tables("hexwide")
    data = counted(items, records)
    sc = yara_amd.Scanner(t)
    matches, rest = sc.string_matches(data, hex=True, wide=True)
    want, want_rest = expected(z, data, sc.verify_calls(data))
    equal(matches, want)
    assert len(rest) == len(want_rest) == 0
    assert len(matches) == records * (items + 1)


def test_one_scanner_alternating():
    man, a = fixture()
    t, z = tables("hexwide")
    data, big = a["data"], counted(3, 300)                # (300 queued: the queue grows)
    fresh = yara_amd.Scanner(t)
    on, off = fresh.string_matches(data, hex=True, wide=True), fresh.string_matches(data, hex=True)
    big_on = yara_amd.Scanner(t).string_matches(big, hex=True, wide=True)
    assert len(big_on[0]) == 300 * 4
    batch = yara_amd.Scanner(t).batch_string_matches([data[:3000], big[:2000]], hex=True)
    sc = yara_amd.Scanner(t)
    for step in ("off", "on", "batch", "big", "on", "off", "big"):
        if step == "batch":
            for wide in (True, False):
                sc.set_hex_wide(wide)
                got = sc.batch_string_matches([data[:3000], big[:2000]], hex=True)
                for x, y in zip(got, batch):
                    np.testing.assert_array_equal(x, y)
            continue
        got = sc.string_matches(big if step == "big" else data, hex=True, wide=step != "off")
        for x, y in zip(got, {"on": on, "off": off, "big": big_on}[step]):
            np.testing.assert_array_equal(x, y)
    for value in (2, -1):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.set_hex_wide(value)
        assert e.value.code == yara_amd.INVALID_ARGUMENT
