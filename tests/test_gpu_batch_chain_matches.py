"""GPU: chained hex strings settled per buffer by the batch match stage
(yr_amd_scanner_set_batch_chains).  The references are the single-block call on each buffer alone
(pinned to stock libyara by tests/golden/chain) and test_gpu_chain_matches' transcription of
scan.c:406-632."""
import functools
import gzip
import os

import numpy as np
import pytest

import yara_amd
from conftest import tables_npz
from test_gpu_chain_matches import (CHAIN, HEX, LIT, NONE, equal, find_events, fixture,
                                    fixture_parts, replay, want_of)

pytestmark = pytest.mark.gpu


def slices_of(man, data):
    """One slice per run of plants of one name, on 1 KiB boundaries."""
    runs = []
    for at, length, note in man["plants"]:
        at += len(data) if at < 0 else 0
        lo, hi, name = at // 1024 * 1024, -(-(at + length) // 1024) * 1024, note.split(":")[0]
        if runs and runs[-1][0] == name:
            runs[-1][2] = hi
        else:
            runs.append([name, lo, hi])
    return [name for name, _, _ in runs], [data[lo:hi] for _, lo, hi in runs]


def check_batch(got, want):
    """got = (matches, match_off, rest, rest_off); want[k] = (matches, rest) of buffer k alone."""
    matches, mo, rest, ro = got
    assert mo[0] == ro[0] == 0 and mo[-1] == len(matches) and ro[-1] == len(rest)
    assert len(mo) == len(ro) == len(want) + 1
    for k, (m, r) in enumerate(want):
        np.testing.assert_array_equal(matches[mo[k]:mo[k + 1]], m, err_msg="matches of %d" % k)
        np.testing.assert_array_equal(rest[ro[k]:ro[k + 1]], r, err_msg="rest of %d" % k)


@pytest.mark.parametrize("hex,wide", [(False, False), (True, False), (True, True)])
def test_fixture_per_buffer(hex, wide):
    import torch
    man, case, z, t = fixture()
    names, bufs = slices_of(man, case["data"])
    assert names.count("dirty") == 1 and "text" in names   # (text: a buffer without a chain record)
    clean = len(bufs)
    bufs = bufs + [case["data"][23552:24576], np.zeros(0, np.uint8)]   # dirty's chain, one result only
    sc, one = yara_amd.Scanner(t), yara_amd.Scanner(t)
    want = [one.string_matches(b, hex=hex, wide=wide, chains=True) for b in bufs]
    got = sc.batch_string_matches(bufs, hex=hex, wide=wide, chains=True)
    check_batch(got, want)
    assert got[1][-1] > sc.batch_string_matches(bufs, hex=hex, wide=wide)[1][-1]
    if hex:   # the per-buffer dirty flag: dirty where the two results are, settled next to it
        d, (head, tail) = names.index("dirty"), man["strings"]["dirty"]
        of = lambda r: z["pool_string"][r["pool_index"]]   # noqa: E731
        plain = one.string_matches(bufs[d], hex=True, wide=wide)[1]
        assert np.isin(of(want[d][1]), [head, tail]).sum() == np.isin(of(plain), [head, tail]).sum() > 2
        assert not (want[d][0]["string"] == head).any()
        assert (want[clean][0]["string"] == head).sum() == 1
        assert not np.isin(of(want[clean][1]), [head, tail]).any()
    if hex and not wide:   # the gather path
        dev = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in bufs]
        check_batch(sc.batch_string_matches_device(dev, hex=True, chains=True), want)


def test_no_chain_across_buffers():
    man, _, z, t = fixture()
    (hs, hb), (ts, tb) = sorted(fixture_parts(z, man["strings"]["two"]).items())
    gap = int(z["str_gap_min"][ts]) + 1
    first, second = np.zeros(512, np.uint8), np.zeros(512, np.uint8)
    first[512 - len(hb):] = np.frombuffer(hb, np.uint8)
    second[gap:gap + len(tb)] = np.frombuffer(tb, np.uint8)
    sc = yara_amd.Scanner(t)
    matches = sc.batch_string_matches([first, second], chains=True)[0]
    assert not (matches["string"] == hs).any()
    whole, _ = sc.string_matches(np.concatenate([first, second]), chains=True)
    assert list(whole["offset"][whole["string"] == hs]) == [512 - len(hb)]


@functools.lru_cache(maxsize=None)
def open_case(heads):
    """test_list_lengths' buffer and its model."""
    man, _, z, _ = fixture()
    parts = fixture_parts(z, man["strings"]["open"])
    (hs, hb), (ts, tb) = sorted(parts.items())
    data = np.zeros(16384, np.uint8)
    for k in range(heads):
        data[1024 + 8 * k:1028 + 8 * k] = np.frombuffer(hb, np.uint8)
    data[9000:9004] = data[12000:12004] = np.frombuffer(tb, np.uint8)
    data[16:20] = np.frombuffer(hb, np.uint8)
    model = replay(find_events(data, parts), z["str_chained_to"], z["str_gap_min"].astype(np.int64),
                   z["str_gap_max"].astype(np.int64))
    assert len(model[hs]) == heads + 1
    return data, want_of(model)


@pytest.mark.parametrize("heads", [1, 63, 64, 65, 511, 512])
def test_group_sizes(heads):
    """A group of heads + 1 list entries (512: the wave's LDS share, 513: the workspace) between
    two groups of other sizes, one of them of the other kind, in one launch."""
    t = fixture()[3]
    sizes = [512 if heads < 512 else 1, heads, 65]
    cases = [open_case(h) for h in sizes]
    matches, mo, rest, ro = yara_amd.Scanner(t).batch_string_matches([c[0] for c in cases], chains=True)
    assert len(rest) == 0 and list(np.diff(mo)) == [h + 1 for h in sizes]
    for k, (_, want) in enumerate(cases):
        equal(matches[mo[k]:mo[k + 1]], want)


@functools.lru_cache(maxsize=None)
def count_case(dropped):
    """test_chain_counts' buffer of 65 chains and its model; `dropped`: a chain without its tail."""
    count = 65
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
        if k != dropped:
            data[far:far + 4] = np.frombuffer(parts[2 * k + 1], np.uint8)
    model = replay(find_events(data, parts), to, np.tile([0, 300], count), np.tile([0, 500], count))
    return data, want_of(model)


@pytest.mark.parametrize("B", [1, 64, None])
def test_group_counts(B):
    """65 groups a buffer, B buffers: B = None makes them more than the replay grid's waves.
    Every seventh buffer lacks one tail, a different one each time."""
    with gzip.open(os.path.join(CHAIN, "chains_65.yarc.gz")) as f:
        sc = yara_amd.Scanner(yara_amd.Tables.from_yarc(f.read(), device=0))
    if B is None:
        B = sc.batch_chain_waves() // 65 + 1
    assert 0 < B <= 256
    cases = [count_case(b % 65 if b % 7 == 3 else -1) for b in range(B)]
    matches, mo, rest, ro = sc.batch_string_matches([c[0] for c in cases], chains=True)
    assert list(np.diff(mo)) == [len(c[1]["offset"]) for c in cases] and len(rest) == 0
    assert mo[1] == sum((k % 5 != 4) * (1 + (k % 3 == 0)) for k in range(65))
    for b, (_, want) in enumerate(cases):
        equal(matches[mo[b]:mo[b + 1]], want)


def test_off_and_refusals():
    _, case, _, t = fixture()
    sc, fresh = yara_amd.Scanner(t), yara_amd.Scanner(t)
    bufs = [case["data"][:16384], case["data"][16384:]]
    want = fresh.batch_string_matches(bufs, hex=True)
    for _ in range(2):   # before and after a call with chains=True
        for x, y in zip(sc.batch_string_matches(bufs, hex=True), want):
            np.testing.assert_array_equal(x, y)
        assert len(sc.batch_string_matches(bufs, hex=True, chains=True)[0]) > len(want[0])
    sc.set_chains(True)   # the single-block setting: not the batch's
    for x, y in zip(sc.batch_string_matches(bufs, hex=True), want):
        np.testing.assert_array_equal(x, y)
    L = yara_amd._lib.lib()
    for h, bad in ((sc._h, 2), (sc._h, -1), (None, 1)):
        assert L.yr_amd_scanner_set_batch_chains(h, bad) == yara_amd._lib.INVALID_ARGUMENT
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(tables_npz("hex"), device=0, strings=True))
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.batch_string_matches(bufs, chains=True)
    assert e.value.code == yara_amd._lib.INVALID_ARGUMENT
