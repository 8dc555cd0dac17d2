"""GPU: loop strings (yr_amd_scanner_set_loops) against stock libyara's lists on tests/golden/loops.
Which records leave the rest comes from the transcription of yr_re_exec in test_alternation_abi."""
import os

import numpy as np
import pytest

import yara_amd
from conftest import GOLDEN
from test_alternation_abi import settle
from test_loops_abi import FIX, fixture

pytestmark = pytest.mark.gpu

LIT, HEX = yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX
_CACHE = {}


def tables(path=os.path.join(FIX, "tables.npz")):
    if path not in _CACHE:
        _CACHE[path] = yara_amd.Tables.from_npz(path, device=0, strings=True)
    return _CACHE[path]


def listed(matches):
    return [tuple(int(m[f]) for f in ("string", "offset", "length", "xor_key")) for m in matches]


def reference():
    """(stock's matches of the strings settled with everything on, the rest then), once: all of
    stock's list but the php call at 1217, whose backward set spans 64 positions."""
    if "ref" not in _CACHE:
        man, a, z = fixture()
        t = tables()
        loop, alt = t.loop_strings(), t.alternation_strings()
        sel = t.match_strings(LIT | HEX) | loop | alt
        php = man["strings"].index("php")
        lost = (a["match_string"] == php) & (a["match_offset"] >= 1153) & (a["match_offset"] <= 1216)
        keep = sel[a["match_string"]] & ~lost
        stock = [tuple(int(x) for x in m) for m in zip(a["match_string"][keep], a["match_offset"][keep],
                                                       a["match_len"][keep], a["match_xor"][keep])]
        calls = yara_amd.Scanner(t).verify_calls(a["data"])
        recs = [(int(r["offset"]), int(r["pool_index"])) for r in calls]
        left = set(settle(z, a["data"], recs, loop | alt, window=False)[1])   # no match: stays
        left.add(recs.index((1217, next(k for o, k in recs if o == 1217 and z["pool_string"][k] == php))))
        gone = np.array([(loop | alt)[z["pool_string"][k]] and r not in left
                         for r, (_, k) in enumerate(recs)])
        _CACHE["ref"] = stock, calls[~gone], (php, 1217)
    return _CACHE["ref"]


def test_fixture_equals_stock():
    man, a, z = fixture()
    stock, want_rest, lost = reference()
    sc = yara_amd.Scanner(tables())
    off = sc.string_matches(a["data"], hex=True, wide=True, alternations=True)
    matches, rest = sc.string_matches(a["data"], hex=True, wide=True, alternations=True, loops=True)
    assert listed(matches) == stock
    np.testing.assert_array_equal(rest, np.array(want_rest, dtype=rest.dtype))
    string = z["pool_string"][rest["pool_index"]]
    assert (int(lost[0]), lost[1]) in set(zip(string.tolist(), rest["offset"].tolist()))
    # with the setting off every loop record is in the rest and none of their matches is out
    loop = tables().loop_strings()
    assert not loop[off[0]["string"]].any() and loop[matches["string"]].sum() > 100
    assert len(off[1]) > len(rest)
    for x, y in zip(off, sc.string_matches(a["data"], hex=True, wide=True, alternations=True)):
        np.testing.assert_array_equal(x, y)                # off again: what it was


@pytest.mark.parametrize("on", [{}, {"wide": True}, {"alternations": True}])
def test_beside_the_other_settings(on):
    a, t = fixture()[1], tables()
    stock, _, _ = reference()
    matches, rest = yara_amd.Scanner(t).string_matches(a["data"], hex=True, loops=True, **on)
    sel = t.match_strings(LIT | HEX) | t.loop_strings()
    if on.get("alternations"):
        sel |= t.alternation_strings()
    assert listed(matches) == [m for m in stock if sel[m[0]]]


def test_chains_beside_and_tables_without_a_loop_string():
    path = os.path.join(GOLDEN, "chain", "tables.npz")
    t, data = tables(path), np.load(os.path.join(GOLDEN, "chain", "case.npz"))["data"]
    assert not t.loop_strings().any()
    sc = yara_amd.Scanner(t)
    for x, y in zip(sc.string_matches(data, hex=True, chains=True),
                    sc.string_matches(data, hex=True, chains=True, loops=True)):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.set_loops(2)
    assert e.value.code == yara_amd.INVALID_ARGUMENT


# (2100: above the fixed grid's 2048 waves -- the stride loop -- and the queue's first capacity)
@pytest.mark.parametrize("records", [0, 1, 65, 2100])
def test_queue_edges(records):
    buf = np.zeros(records * 16 + 64, np.uint8)
    for r in range(records):
        buf[r * 16 + 4:r * 16 + 10 + r % 7] = np.frombuffer(b"Rn6!" + b"a" * (1 + r % 7) + b"z", np.uint8)
    sc = yara_amd.Scanner(tables())
    for data in (buf, buf[:48]):                           # (the same scanner, the grown queue)
        matches, rest = sc.string_matches(data, hex=True, loops=True)
        n = min(records, 3) if data is not buf else records
        assert listed(matches) == [(6, r * 16 + 4, 6 + r % 7, 0) for r in range(n)] and len(rest) == 0


# (window, first byte scanned, end, string, its call): the window ends inside the forward run of
# `run` at 257; it starts inside the backward run of `php`'s call at 1088
@pytest.mark.parametrize("lo,begin,hi,string,at", [(0, 0, 304, "run", 257), (1008, 1024, 1200, "php", 1088)])
def test_window_inside_a_run(lo, begin, hi, string, at):
    import torch
    man, a, z = fixture()
    data, sc = a["data"], yara_amd.Scanner(tables())
    win = torch.zeros(hi - lo + 16, dtype=torch.uint8, device="cuda")
    win[:hi - lo] = torch.from_numpy(data[lo:hi].copy()).cuda()
    torch.cuda.synchronize()
    sc.scan_window(win.data_ptr(), lo, hi, data.size, begin, hi)
    sc.device_result()
    matches, rest = sc.match_device(hex=True, loops=True)
    k = man["strings"].index(string)
    assert k not in matches["string"]
    assert ((z["pool_string"][rest["pool_index"]] == k) & (rest["offset"] == at)).sum() == 1
