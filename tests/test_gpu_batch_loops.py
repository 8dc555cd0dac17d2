"""GPU: loop strings settled per buffer by the batch match stage (yr_amd_scanner_set_batch_loops).
The contract is the single-block call on every buffer alone, classes LITERAL | HEX and
set_loops(1) (test_gpu_loops.py pins that call to stock libyara); the whole fixture as a
one-buffer batch is compared with stock libyara's recorded lists directly."""
import os

import numpy as np
import pytest

import yara_amd
from test_loops_abi import FIX, fixture
from test_gpu_batch_matches import same, singles
from test_gpu_loops import HEX, LIT, listed, reference, tables

pytestmark = pytest.mark.gpu


def contract(t, loops=True, **on):
    """The scanner whose single-block calls are what the batch must give."""
    sc = yara_amd.Scanner(t)
    sc.set_match_classes(LIT | HEX)
    sc.set_loops(loops)
    sc.set_hex_wide(on.get("wide", False))
    sc.set_alternations(on.get("alternations", False))
    return sc


def cut(data, edges):
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


def at(got, k, name, offset):
    """Buffer k's matches of the string `name` at the local offset."""
    m = got[0][int(got[1][k]):int(got[1][k + 1])]
    return m[(m["string"] == fixture()[0]["strings"].index(name)) & (m["offset"] == offset)]


def test_whole_fixture_is_stock():
    man, a, z = fixture()
    stock, want_rest, lost = reference()
    t, data = tables(), a["data"]
    sc = yara_amd.Scanner(t)
    m, mo, rest, ro = sc.batch_string_matches([data], hex=True, wide=True, alternations=True, loops=True)
    assert listed(m) == stock
    assert list(mo) == [0, len(m)] and list(ro) == [0, len(rest)]
    np.testing.assert_array_equal(rest, np.array(want_rest, dtype=rest.dtype))
    string = z["pool_string"][rest["pool_index"]]
    assert (int(lost[0]), lost[1]) in set(zip(string.tolist(), rest["offset"].tolist()))
    off = sc.batch_string_matches([data], hex=True, wide=True, alternations=True)   # off: as today
    same(off, singles(contract(t, loops=False, wide=True, alternations=True), [data]))
    assert not t.loop_strings()[off[0]["string"]].any() and len(off[2]) > len(rest)


# an empty and a 1-byte buffer, `run`'s forward run from 257 cut; inside the backward run of php's
# call at 959; php's call at 1217 reaching back 57 positions only; between coll_g's two .php
CUTS = {"plants": [0, 64, 64, 65, 304, 16384], "backward": [0, 930, 16384],
        "settled": [0, 1160, 16384], "greedy": [0, 646, 16384]}


@pytest.mark.parametrize("name", sorted(CUTS))
def test_cut_into_buffers(name):
    man, a, z = fixture()
    t, data = tables(), a["data"]
    sc = yara_amd.Scanner(t)
    pieces = cut(data, CUTS[name])
    bases = np.array([k * 0x10000 + 3 for k in range(len(pieces))], np.uint64)
    for b in (None, bases):
        got = sc.batch_string_matches(pieces, b, hex=True, loops=True)
        same(got, singles(contract(t), pieces, b))
    whole = sc.batch_string_matches([data], hex=True, loops=True)
    php = man["strings"].index("php")
    if name == "plants":                                  # the bounds are the buffer's: no match at 257
        assert len(pieces[1]) == 0 and len(pieces[2]) == 1 and got[1][2] == got[1][1]
        assert len(at(whole, 0, "run", 257)) == 1 and len(at(got, 3, "run", 257 - 65)) == 0
    if name == "backward":                                # ... and fewer backward results
        count = lambda m, lo: ((m["string"] == php) & (m["offset"] >= lo) & (m["offset"] < lo + 64)).sum()
        assert 0 < count(got[0][int(got[1][1]):], 0) < count(whole[0], 896)
    if name == "settled":                                 # ... 57 of them, where the whole fixture has none
        last = lambda g: g[2][int(g[3][-2]):]             # the last buffer's rest
        left = lambda g, o: ((z["pool_string"][last(g)["pool_index"]] == php) & (last(g)["offset"] == o)).sum()
        assert left(whole, 1217) == 1 and left(got, 57) == 0
        assert all(len(at(got, 1, "php", o)) == 1 for o in (0, 56))
    if name == "greedy":
        assert at(whole, 0, "coll_g", 641)["length"] == 9 and at(got, 0, "coll_g", 641)["length"] == 5


def test_table_sizes():
    man, a, _ = fixture()
    t, data = tables(), a["data"]
    sc, names = yara_amd.Scanner(t), man["strings"]
    last = [data[6400:6400 + 4096]]                       # largest 4096: 4097 words, MATCH at 4096
    got = sc.batch_string_matches(last, hex=True, loops=True)
    same(got, singles(contract(t), last))
    assert at(got, 0, "dot", 0)["length"] == 4096
    word = [data[2048:2048 + 4095], data[:1]]             # 4096 words: MATCH in the table's last word
    got = sc.batch_string_matches(word, hex=True, loops=True)
    same(got, singles(contract(t), word))
    assert at(got, 0, "dot", 0)["length"] == 4095
    small = [data[64:128], data[128:192]]                 # largest 64: 65 words
    got = sc.batch_string_matches(small, hex=True, loops=True)
    same(got, singles(contract(t), small))
    loop = t.loop_strings()[got[0]["string"]]
    want = [("plus", 1, 7), ("star", 10, 7), ("star", 19, 4), ("plus_u", 25, 5), ("star_u", 34, 4),
            ("alt", 1, 9), ("alt", 11, 5)]                # stock's, local
    assert [m[:3] for m in listed(got[0][loop])] == [(names.index(s), o, n) for s, o, n in want]


def test_greedy_replacement_is_per_buffer():
    t, data = tables(), fixture()[1]["data"]
    got = yara_amd.Scanner(t).batch_string_matches([data[640:720]] * 2, hex=True, loops=True)
    same(got, singles(contract(t), [data[640:720]] * 2))
    for k in (0, 1):
        assert at(got, k, "coll_g", 1)["length"] == 9 and at(got, k, "coll_u", 65)["length"] == 5


def test_gaps_are_never_read():
    import torch
    t, data = tables(), fixture()[1]["data"]
    # the fixture in place, cut inside run's forward run from 257: the gap holds bytes of it
    starts = np.array([0, 320], np.uint64)
    sizes = np.array([304, data.size - 320], np.uint64)
    pieces = [data[int(s):int(s + n)] for s, n in zip(starts, sizes)]
    zeroed = data.copy()
    zeroed[304:320] = 0
    sc, got = yara_amd.Scanner(t), []
    for arena in (data, zeroed):
        dev = torch.from_numpy(arena.copy()).cuda()
        torch.cuda.synchronize()
        sc.scan_batch_device(dev.data_ptr(), arena.size, starts, sizes)
        sc.batch_result()
        got.append(sc.match_batch_device(hex=True, loops=True))
        torch.cuda.synchronize()
    same(got[0], got[1])
    same(got[0], singles(contract(t), pieces))


# (2100: above the fixed grid's 2048 waves -- the stride loop -- and the queue's first capacity;
# a record lies within 16 bytes, the cuts every 64 * step: a wave's records straddle buffers)
@pytest.mark.parametrize("records,step", [(1, 1), (65, 3), (2100, 44)])
def test_queue_edges(records, step):
    sc = yara_amd.Scanner(tables())

    def check(n):
        buf = np.zeros(n * 16 + 64, np.uint8)
        for r in range(n):
            buf[r * 16 + 4:r * 16 + 10 + r % 7] = np.frombuffer(b"Rn6!" + b"a" * (1 + r % 7) + b"z", np.uint8)
        size = 64 * step
        edges = list(range(0, buf.size, size)) + [buf.size]
        m, mo, rest, ro = sc.batch_string_matches(cut(buf, edges), hex=True, loops=True)
        assert listed(m) == [(6, (r * 16 + 4) % size, 6 + r % 7, 0) for r in range(n)] and len(rest) == 0
        assert list(np.diff(mo)) == list(np.histogram(np.arange(n) * 16 + 4, bins=edges)[0])

    check(records)
    check(3)                                              # the same scanner, the grown queue


@pytest.mark.parametrize("on", [{}, {"wide": True}, {"alternations": True},
                                {"wide": True, "alternations": True}])
def test_beside_the_other_settings(on):
    t, data = tables(), fixture()[1]["data"]
    pieces = cut(data, [0, data.size // 2, data.size])
    sc = yara_amd.Scanner(t)
    got = sc.batch_string_matches(pieces, hex=True, loops=True, **on)
    same(got, singles(contract(t, **on), pieces))
    assert len(got[0]) > len(sc.batch_string_matches(pieces, hex=True, **on)[0])


def test_settings_are_separate():
    import torch
    t, data = tables(), fixture()[1]["data"]
    pieces = cut(data, CUTS["plants"])
    fresh = yara_amd.Scanner(t)
    off = fresh.batch_string_matches(pieces, hex=True)
    sc = yara_amd.Scanner(t)
    sc.set_batch_loops(True)                              # not the single-block calls' setting
    for x, y in zip(sc.string_matches(data, hex=True), fresh.string_matches(data, hex=True)):
        np.testing.assert_array_equal(x, y)
    same(sc.batch_string_matches(pieces), fresh.batch_string_matches(pieces))   # no hex class: not read
    assert len(sc.batch_string_matches(pieces, hex=True)[0]) > len(off[0])
    sc.set_batch_loops(False)
    sc.set_loops(True)                                    # the single-block setting: not the batch's
    same(sc.batch_string_matches(pieces, hex=True), off)
    for value in (2, -1):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.set_batch_loops(value)
        assert e.value.code == yara_amd.INVALID_ARGUMENT
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(os.path.join(FIX, "tables.npz"), device=0,
                                                     strings=True, regex=False))
    dev = [torch.from_numpy(p.copy()).cuda() for p in pieces[:1]]
    for call, arg in ((bare.batch_string_matches, pieces), (bare.batch_string_matches_device, dev)):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            call(arg, hex=True, loops=True)
        assert e.value.code == yara_amd.INVALID_ARGUMENT


def test_gathered_batch():
    import torch
    from test_gpu_gather import _place
    t = tables()
    pieces = cut(fixture()[1]["data"], CUTS["plants"])
    src, views, host = _place(pieces, [(7 * k + 1) % 16 | 1 for k in range(len(pieces))])
    sc = yara_amd.Scanner(t)
    want = sc.batch_string_matches(pieces, hex=True, loops=True)
    assert len(want[2]) < len(sc.batch_string_matches(pieces, hex=True)[2])
    same(sc.batch_string_matches_device(views, hex=True, loops=True), want)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), host)
