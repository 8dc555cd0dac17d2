"""GPU: alternation strings settled per buffer by the batch match stage
(yr_amd_scanner_set_batch_alternations).  The contract is the single-block call on every buffer
alone, classes LITERAL | HEX and set_alternations(1) (test_gpu_alternation.py pins that call to
stock libyara); the whole fixture as a one-buffer batch is compared with stock libyara's recorded
lists directly."""
import numpy as np
import pytest

import yara_amd
from test_alternation_abi import fixture
from test_gpu_alternation import HEX, LIT, PATHS, case, listed, planted, tables
from test_gpu_batch_matches import same, singles

pytestmark = pytest.mark.gpu


def contract(t, alternations=True, **on):
    """The scanner whose single-block calls are what the batch must give."""
    sc = yara_amd.Scanner(t)
    sc.set_match_classes(LIT | HEX)
    sc.set_alternations(alternations)
    sc.set_hex_wide(on.get("wide", False))
    sc.set_chains(on.get("chains", False))
    return sc


def cut(data, edges):
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


def test_whole_fixture_is_stock():
    man, a, _ = fixture()
    t, z = tables("alternation")
    data, sc = case("alternation"), yara_amd.Scanner(t)
    m, mo, rest, ro = sc.batch_string_matches([data], hex=True, wide=True, alternations=True)
    sel = t.match_strings(LIT | HEX) | t.alternation_strings()
    lost = (man["strings"].index("run65"), 896)           # the only class record left in the rest
    keep = sel[a["match_string"]] & ~((a["match_string"] == lost[0]) & (a["match_offset"] == 896))
    stock = zip(a["match_string"][keep], a["match_offset"][keep], a["match_len"][keep], a["match_xor"][keep])
    assert listed(m) == [tuple(int(x) for x in s) for s in stock]
    assert list(mo) == [0, len(m)] and list(ro) == [0, len(rest)]
    string = z["pool_string"][rest["pool_index"]]
    assert sorted(zip(string[sel[string]], rest["offset"][sel[string]])) == [lost]
    off = sc.batch_string_matches([data], hex=True, wide=True)   # off: what the stage gives today
    same(off, singles(contract(t, alternations=False, wide=True), [data]))
    assert len(off[0]) < len(m) and len(off[2]) > len(rest)


# long_first at 128 runs to 137; `before` at 256: the record at 258 reaches back to 257 and to 256
CUTS = {"plants": [0, 128, 128, 320, 321, 576, 1152, 1600, 16384],
        "long_first": [0, 134, 16384], "before": [0, 257, 16384]}


@pytest.mark.parametrize("name", sorted(CUTS))
def test_cut_into_buffers(name):
    t, z = tables("alternation")
    data, sc = case("alternation"), yara_amd.Scanner(t)
    pieces = cut(data, CUTS[name])
    bases = np.array([k * 0x10000 + 3 for k in range(len(pieces))], np.uint64)
    for b in (None, bases):
        got = sc.batch_string_matches(pieces, b, hex=True, alternations=True)
        same(got, singles(contract(t), pieces, b))
    m = got[0]
    whole = sc.batch_string_matches([data], hex=True, alternations=True)[0]
    names = fixture()[0]["strings"]
    if name == "plants":
        assert len(pieces[1]) == 0 and len(pieces[3]) == 1 and got[1][2] == got[1][1]
    if name == "long_first":                              # the bounds are the buffer's: no match at 128
        s = names.index("long_first")
        assert ((whole["string"] == s) & (whole["offset"] == 128)).any()
        first = m[:int(got[1][1])]
        assert not ((first["string"] == s) & (first["offset"] == 128)).any()
    if name == "before":                                  # ... and one backward result less
        s = names.index("before")
        assert 0 < (m["string"] == s).sum() < (whole["string"] == s).sum()


def test_gaps_are_never_read():
    import torch
    t, z = tables("alternation")
    data = case("alternation")
    # the fixture in place, cut inside long_first's forward run: the gap holds the bytes that complete it
    starts = np.array([0, 144], np.uint64)
    sizes = np.array([134, data.size - 144], np.uint64)
    pieces = [data[int(s):int(s + n)] for s, n in zip(starts, sizes)]
    zeroed = data.copy()
    zeroed[134:144] = 0
    sc, got = yara_amd.Scanner(t), []
    for arena in (data, zeroed):
        dev = torch.from_numpy(arena.copy()).cuda()
        torch.cuda.synchronize()
        sc.scan_batch_device(dev.data_ptr(), arena.size, starts, sizes)
        sc.batch_result()
        got.append(sc.match_batch_device(hex=True, alternations=True))
        torch.cuda.synchronize()
    same(got[0], got[1])
    same(got[0], singles(contract(t), pieces))


# (2100: above the fixed grid's 2048 waves -- the stride loop -- and the queue's first capacity;
# the cuts every 64 * step bytes: a wave's records straddle buffer boundaries)
@pytest.mark.parametrize("records,step", [(1, 1), (65, 3), (2100, 44)])
def test_queue_edges(records, step):
    t, z = tables("alternation")
    sc = yara_amd.Scanner(t)

    def check(n):
        data = planted(n)
        edges = list(range(0, data.size, 64 * step)) + [data.size]
        m, mo, rest, ro = sc.batch_string_matches(cut(data, edges), hex=True, alternations=True)
        assert len(m) == n and len(rest) == 0 and mo[-1] == n
        assert (m["string"] == 0).all() and (m["length"] == 9).all() and (m["offset"] % 64 == 8).all()
        assert list(np.diff(mo)) == list(np.histogram(np.arange(n) * 64 + 8, bins=edges)[0])

    check(records)
    check(3)                                              # the same scanner, the grown queue


@pytest.mark.parametrize("name,on", [("both", {"chains": True}), ("both", {"wide": True, "chains": True}),
                                     ("alternation", {"wide": True})])
def test_with_wide_and_chains(name, on):
    t, z = tables(name)
    data = case(name)
    pieces = cut(data, [0, data.size // 2, data.size])
    sc = yara_amd.Scanner(t)
    got = sc.batch_string_matches(pieces, hex=True, alternations=True, **on)
    same(got, singles(contract(t, **on), pieces))
    assert len(got[0]) > len(sc.batch_string_matches(pieces, hex=True, **on)[0])


def test_settings_are_separate():
    import torch
    t, z = tables("alternation")
    data = case("alternation")
    pieces = cut(data, CUTS["plants"])
    fresh = yara_amd.Scanner(t)
    off = fresh.batch_string_matches(pieces, hex=True)
    sc = yara_amd.Scanner(t)
    sc.set_batch_alternations(True)                       # not the single-block calls' setting
    for x, y in zip(sc.string_matches(data, hex=True), fresh.string_matches(data, hex=True)):
        np.testing.assert_array_equal(x, y)
    same(sc.batch_string_matches(pieces), fresh.batch_string_matches(pieces))   # no hex class: not read
    assert len(sc.batch_string_matches(pieces, hex=True)[0]) > len(off[0])
    sc.set_batch_alternations(False)
    sc.set_alternations(True)                             # the single-block setting: not the batch's
    same(sc.batch_string_matches(pieces, hex=True), off)
    for value in (2, -1):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.set_batch_alternations(value)
        assert e.value.code == yara_amd.INVALID_ARGUMENT
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(PATHS["alternation"], device=0, strings=True,
                                                     regex=False))
    dev = [torch.from_numpy(p.copy()).cuda() for p in pieces[:1]]
    for call, arg in ((bare.batch_string_matches, pieces), (bare.batch_string_matches_device, dev)):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            call(arg, hex=True, alternations=True)
        assert e.value.code == yara_amd.INVALID_ARGUMENT


def test_gathered_batch():
    import torch
    from test_gpu_gather import _place
    t, z = tables("alternation")
    pieces = cut(case("alternation"), CUTS["plants"])
    src, views, host = _place(pieces, [(7 * k + 1) % 16 | 1 for k in range(len(pieces))])
    sc = yara_amd.Scanner(t)
    want = sc.batch_string_matches(pieces, hex=True, alternations=True)
    assert len(want[2]) < len(sc.batch_string_matches(pieces, hex=True)[2])
    same(sc.batch_string_matches_device(views, hex=True, alternations=True), want)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), host)
