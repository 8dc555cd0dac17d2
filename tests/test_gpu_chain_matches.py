"""GPU: chained hex strings settled by the match stage (yr_amd_scanner_set_chains) against stock
libyara's match lists (tests/golden/chain, hex_1M) and a transcription of scan.c:406-632 that
equals them there."""
import gzip
import json
import os

import numpy as np
import pytest

import yara_amd
from conftest import GOLDEN, REPO, case_data, golden, tables_npz

pytestmark = pytest.mark.gpu

LIT, HEX = yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX
FIELDS = ("string", "offset", "length", "xor_key")
CHAIN = os.path.join(GOLDEN, "chain")
NONE = 0xFFFFFFFF
_CACHE = {}


def fixture():
    if not _CACHE:
        with open(os.path.join(CHAIN, "manifest.json")) as f:
            _CACHE["man"] = json.load(f)
        _CACHE["case"] = dict(np.load(os.path.join(CHAIN, "case.npz")))
        _CACHE["z"] = dict(np.load(os.path.join(CHAIN, "tables.npz")))
        _CACHE["tables"] = yara_amd.Tables.from_npz(os.path.join(CHAIN, "tables.npz"), device=0,
                                                    strings=True)
    return _CACHE["man"], _CACHE["case"], _CACHE["z"], _CACHE["tables"]


def stock(case, strings):
    keep = np.isin(case["match_string"], strings)
    return {"string": case["match_string"][keep], "offset": case["match_offset"][keep],
            "length": case["match_len"][keep], "xor_key": case["match_xor"][keep]}


def equal(got, want):
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def replay(events, to, gmin, gmax):
    """_yr_scan_verify_chained_string_match over (string, offset, length) events in call order:
    {head: [(offset, length)]}, each list ascending with the first match of an offset kept."""
    tail = {k for k in range(len(to)) if to[k] != NONE and k not in set(to)}
    unconfirmed, matches = {}, {}   # string -> [[offset, length, chain_length]] ascending

    def add(lst, m):   # _yr_scan_add_match_to_list, replace_if_exists == 0
        if all(e[0] != m[0] for e in lst):
            lst.append(m)
            lst.sort(key=lambda e: e[0])

    def in_gap(m, s, offset):
        return m[0] + m[1] + gmax[s] >= offset and m[0] + m[1] + gmin[s] <= offset

    def update(s, m, n):   # _yr_scan_update_match_chain_length
        if m[2] == n:
            return
        m[2] = n
        if to[s] != NONE:
            for e in unconfirmed.get(to[s], []):
                if in_gap(e, s, m[0]):
                    update(to[s], e, n + 1)

    for s, offset, length in events:
        add_match = to[s] == NONE
        if not add_match:
            own, prev = unconfirmed.get(s, []), unconfirmed.setdefault(to[s], [])
            lowest = own[0][0] if own else offset
            for m in list(prev):
                if m[0] + m[1] + gmax[s] < lowest:
                    prev.remove(m)
                elif in_gap(m, s, offset):
                    add_match = True
                    break
        if not add_match:
            continue
        if s not in tail:
            add(unconfirmed.setdefault(s, []), [offset, length, 0])
            continue
        for m in unconfirmed[to[s]]:
            if in_gap(m, s, offset):
                update(to[s], m, 1)
        head, full = s, 0
        while to[head] != NONE:
            head, full = to[head], full + 1
        for m in list(unconfirmed[head]):
            if m[2] == full:
                unconfirmed[head].remove(m)
                add(matches.setdefault(head, []), [m[0], offset - m[0] + length])
    return {k: [tuple(m) for m in v] for k, v in matches.items()}


def find_events(data, parts):
    """The events of literal parts {string: bytes} in a buffer, in call order (by position)."""
    raw = bytes(data)
    ev = []
    for s, b in parts.items():
        at = raw.find(b)
        while at >= 0:
            ev.append((at, s, len(b)))
            at = raw.find(b, at + 1)
    return [(s, at, n) for at, s, n in sorted(ev)]


def fixture_parts(z, strings):
    off = z["str_offsets"]
    return {s: bytes(z["str_bytes"][off[s]:off[s + 1]]) for s in strings}


def want_of(model):
    rows = sorted((h, o, n) for h, v in model.items() for o, n in v)
    return {"string": np.array([r[0] for r in rows], np.uint64),
            "offset": np.array([r[1] for r in rows], np.uint64),
            "length": np.array([r[2] for r in rows], np.uint64), "xor_key": np.zeros(len(rows))}


def test_transcription_equals_stock():
    man, case, z, _ = fixture()
    lit = [s for n in ("two", "three", "open") for s in man["strings"][n]]
    model = replay(find_events(case["data"], fixture_parts(z, lit)), z["str_chained_to"],
                   z["str_gap_min"].astype(np.int64), z["str_gap_max"].astype(np.int64))
    equal(want_of(model), stock(case, lit))
    assert len(model) == 3 and sum(map(len, model.values())) == 14


def test_fixture_matches_and_rest():
    man, case, z, t = fixture()
    settled = t.chain_strings(LIT | HEX)
    assert sorted(np.nonzero(settled)[0]) == sorted(
        s for n in ("two", "three", "open", "wild", "dirty", "vary") for s in man["strings"][n])
    dirty = [s for n in man["dirty"] for s in man["strings"][n]]
    heads = [man["strings"][n][0] for n in ("two", "three", "open", "wild", "vary")]
    sc = yara_amd.Scanner(t)
    plain, plain_rest = sc.string_matches(case["data"], hex=True)
    got, rest = sc.string_matches(case["data"], hex=True, chains=True)
    classes = list(np.nonzero(t.match_strings(LIT | HEX))[0])
    equal(got, stock(case, classes + heads))
    assert len(got) == len(plain) + 16
    # the rest: the calls of everything else, in order -- the dirty chain's all among them
    gone = settled[z["pool_string"][plain_rest["pool_index"]]] & \
        ~np.isin(z["pool_string"][plain_rest["pool_index"]], dirty)
    np.testing.assert_array_equal(rest, plain_rest[~gone])
    assert np.isin(z["pool_string"][rest["pool_index"]], dirty).sum() == \
        np.isin(z["pool_string"][plain_rest["pool_index"]], dirty).sum() > 0


def test_fixture_literal_class_leaves_unsettled_chains():
    """With the literal class alone the chains with a hex part (wild, dirty, vary) and the
    regexp's chain are unsettled: their records stay in the rest, in place, and yield nothing."""
    man, case, z, t = fixture()
    settled = t.chain_strings(LIT)
    unsettled = [s for n in ("wild", "dirty", "vary", "regexp") for s in man["strings"][n]]
    assert not settled[unsettled].any()
    sc = yara_amd.Scanner(t)
    plain, plain_rest = sc.string_matches(case["data"])
    got, rest = sc.string_matches(case["data"], chains=True)
    heads = [man["strings"][n][0] for n in ("two", "three", "open")]
    equal(got, stock(case, list(np.nonzero(t.match_strings(LIT))[0]) + heads))
    assert len(got) == len(plain) + 14 and not np.isin(got["string"], unsettled).any()
    of = z["pool_string"][plain_rest["pool_index"]]
    np.testing.assert_array_equal(rest, plain_rest[~settled[of]])
    assert np.isin(z["pool_string"][rest["pool_index"]], unsettled).sum() == np.isin(of, unsettled).sum() >= 8


def test_hex_1m_chain():
    rec = golden()["cases"]["hex_1M"]
    arr = np.load(os.path.join(REPO, "tests", "golden", "cases", "hex_1M.npz"))
    with gzip.open(os.path.join(GOLDEN, "yarc", "hex.yarc.gz")) as f:
        t = yara_amd.Tables.from_yarc(f.read(), device=0)
    got, rest = yara_amd.Scanner(t).string_matches(case_data(rec), chains=True)
    nine = arr["match_string"] == 9
    assert nine.sum() == 6
    np.testing.assert_array_equal(got["offset"][got["string"] == 9], arr["match_offset"][nine])
    np.testing.assert_array_equal(got["length"][got["string"] == 9], arr["match_len"][nine])
    ps = dict(np.load(tables_npz("hex")))["pool_string"]
    assert not np.isin(ps[rest["pool_index"]], [9, 10]).any()


@pytest.mark.parametrize("heads", [1, 63, 64, 65, 130, 511, 512])
def test_list_lengths(heads):
    """`heads` + 1 unconfirmed heads of the unbounded chain, appended in ascending order, in
    reach of one late tail; a second tail finds nothing.  511 fills the wave's LDS share (512
    entries), 512 takes the lists to the workspace.  (Inserts below the list's end:
    test_insert_positions.)"""
    man, _, z, t = fixture()
    parts = fixture_parts(z, man["strings"]["open"])
    (hs, hb), (ts, tb) = sorted(parts.items())
    data = np.zeros(16384, np.uint8)
    for k in range(heads):
        data[1024 + 8 * k:1028 + 8 * k] = np.frombuffer(hb, np.uint8)
    data[9000:9004] = np.frombuffer(tb, np.uint8)
    data[16:20] = np.frombuffer(hb, np.uint8)
    data[12000:12004] = np.frombuffer(tb, np.uint8)
    model = replay(find_events(data, parts), z["str_chained_to"], z["str_gap_min"].astype(np.int64),
                   z["str_gap_max"].astype(np.int64))
    assert len(model[hs]) == heads + 1
    got, rest = yara_amd.Scanner(t).string_matches(data, chains=True)
    equal(got, want_of(model))
    assert len(rest) == 0


D = 6000   # the hand-made pool entry's backtrack


@pytest.fixture(scope="module")
def hand_made(tmp_path_factory):
    """The fixture's tables with the pool entry of `two`'s head handed to `open`'s head, backtrack
    D: the atom 10 11 12 13 ending at position i is then a call of `open`'s head at offset i - D
    with length D (FITS_IN_ATOM: scan.c:912).  No compiled file has such an entry -- a part's
    offsets ascend in record order there, equal at most -- it drives the ordered insert's count,
    duplicate test and shift through the wave."""
    man, _, z, _ = fixture()
    two, head = man["strings"]["two"][0], man["strings"]["open"][0]
    z = dict(z)
    k = np.nonzero(z["pool_string"] == two)[0]
    assert len(k) == 1
    z["pool_string"], z["pool_backtrack"] = z["pool_string"].copy(), z["pool_backtrack"].copy()
    z["pool_string"][k], z["pool_backtrack"][k] = head, D
    path = str(tmp_path_factory.mktemp("chain") / "hand_made.npz")
    np.savez(path, **z)
    return z, yara_amd.Tables.from_npz(path, device=0, strings=True)


@pytest.mark.parametrize("where", ["front", "middle", "step", "equal"])
@pytest.mark.parametrize("heads", [63, 64, 65, 130])
def test_insert_positions(hand_made, heads, where):
    """A list of `heads` entries at 1024 + 8 k, then a call whose offset lies below them all, in
    the middle, right below entry 64 (the sweep's step; past the end for shorter lists) or on
    an entry's offset (dropped); two tails.  The events are the device's own records."""
    man, _, _, _ = fixture()
    z, t = hand_made
    head, tail = man["strings"]["open"]
    target = {"front": 1020, "middle": 1024 + 8 * (heads // 2) + 1, "step": 1024 + 8 * 64 - 3,
              "equal": 1024 + 8 * (heads // 2)}[where]
    data = np.zeros(16384, np.uint8)
    for k in range(heads):
        data[1024 + 8 * k:1028 + 8 * k] = [0x30, 0x31, 0x32, 0x33]
    data[target + D - 4:target + D] = [0x10, 0x11, 0x12, 0x13]
    data[14000:14004] = data[15000:15004] = [0x34, 0x35, 0x36, 0x37]
    sc = yara_amd.Scanner(t)
    recs = sc.verify_calls(data)
    of = z["pool_string"][recs["pool_index"]]
    length = np.where(of == head, z["pool_backtrack"][recs["pool_index"]], 4)
    events = [(s, int(o), int(n)) for s, o, n in zip(of, recs["offset"], length) if s in (head, tail)]
    assert len(events) == heads + 3 and events[heads] == (head, target, D)
    model = replay(events, z["str_chained_to"], z["str_gap_min"].astype(np.int64),
                   z["str_gap_max"].astype(np.int64))
    assert len(model[head]) == heads + (where != "equal")
    got, rest = sc.string_matches(data, chains=True)
    equal(got, want_of(model))
    assert len(rest) == 0


@pytest.mark.parametrize("count", [1, 64, 65])
def test_chain_counts(count):
    """`count` two-part chains (make_chain.py chain_rules), eight to a stretch of 800 bytes with
    their events interleaved; every third chain has a second head, every fifth a tail out of range."""
    with gzip.open(os.path.join(CHAIN, "chains_%d.yarc.gz" % count)) as f:
        t = yara_amd.Tables.from_yarc(f.read(), device=0)
    assert t.chain_strings(LIT).all() and t.string_count() == 2 * count
    data = np.zeros(8192, np.uint8)
    parts, to = {}, np.full(2 * count, NONE, np.uint64)
    for k in range(count):
        parts[2 * k], parts[2 * k + 1] = bytes([0xC0, k >> 8, k & 255, 1]), bytes([0xC0, k >> 8, k & 255, 2])
        to[2 * k + 1] = 2 * k
        at = 16 + 800 * (k // 8) + 24 * (k % 8)
        data[at:at + 4] = np.frombuffer(parts[2 * k], np.uint8)
        if k % 3 == 0:
            data[at - 8:at - 4] = np.frombuffer(parts[2 * k], np.uint8)
        far = at + 4 + (520 if k % 5 == 4 else 300) + 3 * (k % 8)
        data[far:far + 4] = np.frombuffer(parts[2 * k + 1], np.uint8)
    gaps = np.tile([0, 300], count), np.tile([0, 500], count)
    model = replay(find_events(data, parts), to, *gaps)
    got, rest = yara_amd.Scanner(t).string_matches(data, chains=True)
    equal(got, want_of(model))
    assert len(got) == sum((k % 5 != 4) * (1 + (k % 3 == 0)) for k in range(count))
    assert len(rest) == 0


def test_chains_off_and_refusals():
    man, case, z, t = fixture()
    sc, fresh = yara_amd.Scanner(t), yara_amd.Scanner(t)
    want, want_rest = fresh.string_matches(case["data"], hex=True)
    for _ in range(2):   # before and after a call with chains=True
        got, rest = sc.string_matches(case["data"], hex=True)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(rest, want_rest)
        assert len(sc.string_matches(case["data"], hex=True, chains=True)[0]) > len(want)
    L = yara_amd._lib.lib()
    for bad in (2, -1):
        assert L.yr_amd_scanner_set_chains(sc._h, bad) == yara_amd._lib.INVALID_ARGUMENT
    # a window that is not the whole block: every chain record stays in the rest
    import torch
    dev = torch.from_numpy(case["data"].copy()).cuda()
    size = dev.numel()
    sc.set_chains(True)
    sc.set_match_classes(LIT | HEX)
    for lo, hi in ((0, size), (0, size - 4096)):
        results = []
        for on in (True, False):
            sc.set_chains(on)
            sc.scan_window(dev.data_ptr(), 0, hi, size, 0, hi)
            sc.device_result()
            results.append(sc.match_device())
        (got, rest), (off, off_rest) = results
        if hi == size:
            assert len(got) > len(off) and len(rest) < len(off_rest)
        else:   # a shard: what the call gives with chains off
            np.testing.assert_array_equal(got, off)
            np.testing.assert_array_equal(rest, off_rest)
            assert t.chain_strings(LIT | HEX)[z["pool_string"][rest["pool_index"]]].sum() > 20
    sc.set_chains(True)
    # the batch calls never read the setting
    b0 = fresh.batch_string_matches([case["data"]], hex=True)
    b1 = sc.batch_string_matches([case["data"]], hex=True)
    for x, y in zip(b0, b1):
        np.testing.assert_array_equal(x, y)
    # chains on, no chain records on the tables
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(tables_npz("hex"), device=0, strings=True))
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.string_matches(case["data"], chains=True)
    assert e.value.code == yara_amd._lib.INVALID_ARGUMENT
