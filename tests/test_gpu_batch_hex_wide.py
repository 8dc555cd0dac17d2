"""GPU: the batch's wave-wide path (yr_amd_scanner_set_batch_hex_wide).  The contract is the
single-block call on every buffer alone, classes LITERAL | HEX and set_hex_wide(1)
(test_gpu_hex_wide.py pins that call to stock libyara); the whole fixture as a one-buffer
batch is compared with stock libyara's recorded lists directly."""
import numpy as np
import pytest

import yara_amd
from test_gpu_batch_matches import same, singles
from test_gpu_hex_wide import HEX, LIT, counted, equal, fixture, stock, tables
from test_hex_match_abi import class_rule

pytestmark = pytest.mark.gpu


def contract(t, wide=True):
    """The scanner whose single-block calls are what a wide batch must give."""
    sc = yara_amd.Scanner(t)
    sc.set_match_classes(LIT | HEX)
    sc.set_hex_wide(wide)
    return sc


def cut(data, edges):
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


def test_whole_fixture_is_stock():
    man, a = fixture()
    t, z = tables("hexwide")
    data, names = a["data"], man["strings"]
    sc = yara_amd.Scanner(t)
    m, mo, rest, ro = sc.batch_string_matches([data], hex=True, wide=True)
    order = [(names.index("order"), 3072), (names.index("order_narrow"), 3328)]
    equal(m, stock(a, z, drop=order))
    assert list(mo) == [0, len(m)] and list(ro) == [0, len(rest)]
    string = z["pool_string"][rest["pool_index"]]
    in_class = class_rule(z["str_flags"], LIT | HEX)[string]
    assert in_class.sum() == man["order_excluded"] == len(order)
    assert sorted(zip(string[in_class], rest["offset"][in_class])) == order
    assert 4096 + 4 in m["length"][m["string"] == names.index("limit")]
    # off: what the batch hex stage gives today -- the wide records are in the rest
    off = sc.batch_string_matches([data], hex=True)
    same(off, singles(contract(t, wide=False), [data]))
    assert {0, 2, 3, 5, 8} <= set(z["pool_string"][off[2]["pool_index"]])
    assert len(off[0]) < len(m)


# plants (manifest): fwd 896 (continuation at 1000), back70 1792..1997, limit 8192..12396
CUTS = {"plants": [0, 512, 512, 1280, 1281, 2048, 3072, 4608, 8192, 49152],
        "back": [0, 1892, 49152],        # the buffer's start limits the backward run
        "fwd": [0, 990, 49152],          # the continuation lies in the next buffer
        "limit": [0, 8000, 12500, 49152]}


@pytest.mark.parametrize("name", sorted(CUTS))
def test_cut_into_buffers(name):
    man, a = fixture()
    t, z = tables("hexwide")
    pieces = cut(a["data"], CUTS[name])
    sc = yara_amd.Scanner(t)
    bases = np.array([k * 0x10000 + 3 for k in range(len(pieces))], np.uint64)
    for b in (None, bases):
        got = sc.batch_string_matches(pieces, b, hex=True, wide=True)
        same(got, singles(contract(t), pieces, b))
    m, mo = got[0], got[1]
    first = m[:int(mo[1])]
    whole = sc.batch_string_matches([a["data"]], hex=True, wide=True)[0]
    names = man["strings"]
    if name == "fwd":
        assert ((whole["string"] == 0) & (whole["offset"] == 896)).any()
        assert not ((first["string"] == 0) & (first["offset"] == 896)).any()
    if name == "back":
        s = names.index("back70")
        assert 0 < (m["string"] == s).sum() < (whole["string"] == s).sum()
    if name == "limit":
        mid = m[int(mo[1]):int(mo[2])]
        assert 4096 + 4 in mid["length"][mid["string"] == names.index("limit")]
    if name == "plants":
        assert mo[2] == mo[1] and len(pieces[1]) == 0 and len(pieces[3]) == 1


def test_gaps_are_never_read():
    import torch
    data = fixture()[1]["data"]
    t, z = tables("hexwide")
    # the fixture in place, cut inside the fwd plant's reach and inside back70's: the gaps
    # and the neighbours hold exactly the bytes that complete the cut plants
    starts = np.array([0, 992, 1904], np.uint64)
    sizes = np.array([981, 901, data.size - 1904], np.uint64)
    pieces = [data[int(s):int(s + n)] for s, n in zip(starts, sizes)]
    zeroed = data.copy()
    zeroed[981:992] = 0
    zeroed[1893:1904] = 0
    sc, got = yara_amd.Scanner(t), []
    for arena in (data, zeroed):
        dev = torch.from_numpy(arena.copy()).cuda()
        torch.cuda.synchronize()
        sc.scan_batch_device(dev.data_ptr(), arena.size, starts, sizes)
        sc.batch_result()
        got.append(sc.match_batch_device(hex=True, wide=True))
        torch.cuda.synchronize()
    same(got[0], got[1])
    same(got[0], singles(contract(t), pieces))


@pytest.mark.parametrize("items,records,step", [
    (1, 1, 1), (64, 1, 1), (65, 1, 1), (200, 1, 1),
    (3, 4, 1),          # the same (string, local offset) in every buffer: a match each
    (3, 64, 3), (3, 65, 3),   # a wave's records straddle buffer boundaries
    (3, 300, 44)])      # more than the queue's first capacity: it grows, the pass reruns
def test_counts(items, records, step):
    t, z = tables("hexwide")
    data = counted(items, records)
    edges = list(range(0, records * 512, step * 512)) + [data.size]
    pieces = cut(data, edges) + [data[:0], data[:700]]
    got = yara_amd.Scanner(t).batch_string_matches(pieces, hex=True, wide=True)
    same(got, singles(contract(t), pieces))
    assert len(got[2]) == 0
    assert len(got[0]) == (records + 1) * (items + 1)


@pytest.mark.parametrize("first", ["single", "batch300"])
def test_repeated_calls_after_another_queue_layout(first):
    """The queue the single-block driver, or a batch of 300 wide records, left behind
    serves the batch calls that follow: the same results call after call."""
    t, z = tables("hexwide")
    data = counted(3, 300)
    pieces = cut(data, list(range(0, 300 * 512, 44 * 512)) + [data.size])
    want = yara_amd.Scanner(t).batch_string_matches(pieces, hex=True, wide=True)
    sc = yara_amd.Scanner(t)
    if first == "single":
        assert len(sc.string_matches(data[:2000], hex=True, wide=True)[0]) > 0
    for _ in range(6):
        same(sc.batch_string_matches(pieces, hex=True, wide=True), want)


def test_gathered_batch():
    import torch
    from test_gpu_gather import _place
    data = fixture()[1]["data"]
    t, z = tables("hexwide")
    pieces = cut(data, CUTS["plants"])
    src, views, host = _place(pieces, [(7 * k + 1) % 16 | 1 for k in range(len(pieces))])
    sc = yara_amd.Scanner(t)
    want = sc.batch_string_matches(pieces, hex=True, wide=True)
    assert len(want[0]) > 20 and len(want[2]) < len(sc.batch_string_matches(pieces, hex=True)[2])
    same(sc.batch_string_matches_device(views, hex=True, wide=True), want)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), host)


def test_one_scanner_alternating():
    data = fixture()[1]["data"]
    t, z = tables("hexwide")
    pieces = cut(data, CUTS["plants"])
    on = yara_amd.Scanner(t).batch_string_matches(pieces, hex=True, wide=True)
    off = yara_amd.Scanner(t).batch_string_matches(pieces, hex=True)
    single = {w: contract(t, w).string_matches(data) for w in (True, False)}
    assert len(on[0]) > len(off[0]) and len(on[2]) < len(off[2])
    sc = yara_amd.Scanner(t)
    for step in ("on", "off", "single", "off", "on", "set", "single", "on"):
        if step == "set":        # each setting affects only its own calls
            sc.set_batch_hex_wide(True)
            for x, y in zip(sc.string_matches(data, hex=True), single[False]):
                np.testing.assert_array_equal(x, y)
            same(sc.batch_string_matches(pieces, hex=True), on)
            same(sc.batch_string_matches(pieces), yara_amd.Scanner(t).batch_string_matches(pieces))
            sc.set_batch_hex_wide(False)
            sc.set_hex_wide(True)
            same(sc.batch_string_matches(pieces, hex=True), off)
            sc.set_hex_wide(False)
        elif step == "single":
            for x, y in zip(sc.string_matches(data, hex=True, wide=True), single[True]):
                np.testing.assert_array_equal(x, y)
        else:
            same(sc.batch_string_matches(pieces, hex=True, wide=step == "on"), on if step == "on" else off)
    for value in (2, -1):
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.set_batch_hex_wide(value)
        assert e.value.code == yara_amd.INVALID_ARGUMENT
