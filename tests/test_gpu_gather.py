"""Batches of buffers scattered in device memory: the gather kernel
(yr_amd_batch_gather) byte for byte, and yr_amd_scan_batch_gather_device against
the host batch path, the oracle and the single-block call.

The sources of every test lie in ONE torch uint8 device tensor filled with
0xA5: piece k at an offset that gives its address a prescribed value mod 16,
at least one filler byte between two pieces.
"""
import functools

import numpy as np
import pytest

import oracle
import yara_amd
from yara_amd import _hip, _lib
from conftest import case_data, golden, ref_tables, tables_npz

pytestmark = pytest.mark.gpu

CHUNK = 8192      # bytes of the arena one wave packs per step (batch.h kGatherChunk * 16)
FILL = 0xA5
GUARD = 64

# table set -> (golden case, bytes of it used)  (test_gpu_batch.py's)
CASES = {
    "C": ("C_planted16M", 1 << 20),
    "lit": ("lit_1M", 1 << 20),
    "short": ("short_1M", 1 << 18),
    "rx": ("rx_1M", 1 << 19),
}
SIZES = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 70001]


@functools.lru_cache(maxsize=None)
def _data(name):
    case, n = CASES[name]
    d = case_data(golden()["cases"][case])[:n].copy()
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref(name):
    return ref_tables(name)


@functools.lru_cache(maxsize=None)
def _scanner(name):
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    return yara_amd.Scanner(tab)


def _sync():
    assert _hip.hip().hipDeviceSynchronize() == 0


def _place(pieces, mis):
    """(source tensor, views): piece k's bytes at an address congruent to
    mis[k] mod 16 inside one device tensor of 0xA5; views[k] is that slice."""
    import torch
    total = sum(len(p) + 17 for p in pieces) + 32
    t = torch.empty(total, dtype=torch.uint8, device="cuda")
    base = t.data_ptr() % 16
    host = np.full(total, FILL, np.uint8)
    offs, at = [], 1
    for p, m in zip(pieces, mis):
        at += (m - base - at) % 16
        offs.append(at)
        host[at:at + len(p)] = p
        at += len(p) + 1            # (a filler byte behind every piece)
    assert at <= total
    t.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()        # (the scanner runs on a stream of its own)
    views = [t[o:o + len(p)] for o, p in zip(offs, pieces)]
    for v, m, p in zip(views, mis, pieces):
        # (torch gives an empty slice no address)
        assert v.numel() == len(p) and (len(p) == 0 or v.data_ptr() % 16 == m)
    return t, views, host


def _unchanged(t, host):
    assert np.array_equal(t.cpu().numpy(), host), "the gather wrote to its sources"


def _packed(pieces, starts, arena_size):
    want = np.zeros(arena_size, np.uint8)
    for p, s in zip(pieces, starts):
        want[int(s):int(s) + len(p)] = p
    return want


def _random_pieces(sizes, seed):
    rng = np.random.default_rng(seed)
    # (no zero bytes: a gap that should be zero cannot pass for data)
    return [rng.integers(1, 256, int(s)).astype(np.uint8) for s in sizes]


def _gather_and_check(pieces, mis, starts, arena_size):
    import torch
    src, views, host = _place(pieces, mis)
    arena = torch.full((arena_size + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    # (an empty buffer's address: null, or any address)
    ptrs = [v.data_ptr() if v.numel() else (k % 2) * (src.data_ptr() + k % 16)
            for k, v in enumerate(views)]
    _scanner("C").batch_gather(arena.data_ptr(), arena_size, starts, ptrs, [len(p) for p in pieces])
    _sync()
    got = arena.cpu().numpy()
    want = _packed(pieces, starts, arena_size)
    bad = np.flatnonzero(got[:arena_size] != want)
    assert len(bad) == 0, "first differing arena byte: %d of %d" % (bad[0], arena_size)
    assert np.all(got[arena_size:] == 0xFF), "bytes at or beyond arena_size were written"
    _unchanged(src, host)


# -- 1. the pack, byte for byte -----------------------------------------------------

@pytest.mark.parametrize("last", [5, 32])
def test_pack_every_misalignment_and_size(last):
    """Source misalignments 0..15 x sizes around 16, 32 and 4096 and one of many
    chunks; an arena_size that is no multiple of 16 (last buffer of 5 bytes:
    the last granule takes the narrow stores) and one that is."""
    sizes = [s for m in range(16) for s in SIZES] + [last]
    mis = [m for m in range(16) for _ in SIZES] + [7]
    starts, arena = yara_amd.batch_layout(sizes)
    assert (arena % 16 != 0) == (last == 5)
    assert max(SIZES) >= 3 * CHUNK          # (a buffer over at least 3 chunks)
    _gather_and_check(_random_pieces(sizes, 1), mis, starts, arena)


def test_pack_empty_buffers_share_a_start():
    sizes = [5, 0, 0, 7]
    starts, arena = yara_amd.batch_layout(sizes)
    assert list(starts) == [0, 16, 16, 16] and arena == 23
    _gather_and_check(_random_pieces(sizes, 2), [3, 0, 9, 15], starts, arena)
    # an empty buffer last, and only empty buffers
    _gather_and_check(_random_pieces([17, 0], 3), [1, 2], [0, 32], 40)
    _gather_and_check(_random_pieces([0, 0], 3), [0, 5], [0, 0], 0)
    _gather_and_check(_random_pieces([0, 0], 3), [0, 5], [16, 48], 100)


def test_pack_no_buffers():
    """n = 0: an arena of zeros (and nothing at all for an empty arena)."""
    for arena in (0, 1, 16, 100, 3 * CHUNK + 9):
        _gather_and_check([], [], [], arena)


def test_pack_caller_chosen_starts():
    """Gaps of 16..47 bytes before every buffer and one gap longer than a
    chunk (a chunk of nothing but zeros), the arena ending in a gap."""
    rng = np.random.default_rng(4)
    sizes = [int(s) for s in rng.integers(0, 200, 60)] + [3 * CHUNK + 5, 1, 16, 33]
    starts, at = [], 0
    for k, s in enumerate(sizes):
        at += 16 + 16 * int(rng.integers(0, 2))          # 16 or 32, + the alignment padding
        if k == 30:
            at += 2 * CHUNK + 16                         # the long gap
        starts.append(at)
        at = (at + s + 15) // 16 * 16
    gaps = np.array(starts[1:]) - (np.array(starts[:-1]) + np.array(sizes[:-1]))
    assert gaps.min() >= 16 and np.sort(gaps)[-2] <= 47 and gaps.max() > CHUNK
    _gather_and_check(_random_pieces(sizes, 5), [int(m) for m in rng.integers(0, 16, len(sizes))],
                      starts, at + 40)


def test_pack_many_buffers_in_one_chunk():
    """More than 300 buffers, empty ones among them, inside one chunk; then one
    buffer over several chunks."""
    rng = np.random.default_rng(6)
    sizes = [int(s) for s in rng.integers(0, 17, 340)] + [4 * CHUNK + 3]
    starts, arena = yara_amd.batch_layout(sizes)
    ends = starts + np.array(sizes, np.uint64)
    inside = (starts // CHUNK == 0) & (ends <= CHUNK)
    assert np.count_nonzero(inside) >= 300 and np.count_nonzero(inside & (ends > starts)) >= 300
    assert (int(ends[-1]) - 1) // CHUNK - int(starts[-1]) // CHUNK >= 3
    _gather_and_check(_random_pieces(sizes, 7), [k % 16 for k in range(len(sizes))], starts, arena)


def test_gather_rejects_bad_arguments():
    import torch
    sc = _scanner("C")
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for starts, sizes, ptrs, arena, size in (
            ([0, 8], [4, 4], [p, p], p, 4096),          # start not 16-byte aligned
            ([16, 0], [4, 4], [p, p], p, 4096),         # not ascending
            ([0, 16], [17, 4], [p, p], p, 4096),        # overlap
            ([0, 4080], [4, 17], [p, p], p, 4096),      # past the arena
            ([0], [4], [p], p + 8, 4000),               # arena not aligned
            ([0], [4], [p], p, 1 << 32),                # arena of 4 GiB
            ([0, 16], [4, 4], [p, 0], p, 4096)):        # a null buffer of a non-zero size
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.batch_gather(arena, size, starts, ptrs, sizes)
        assert e.value.code == _lib.INVALID_ARGUMENT
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.scan_batch_gather_device([p, 0], [4, 4])
    assert e.value.code == _lib.INVALID_ARGUMENT
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sc.batch_gather(a.data_ptr(), 4096, [0, 16], [p, 0], [4, 0])   # (a null EMPTY buffer is fine)
    _sync()


# -- 2. results equal the host batch path ----------------------------------------------

def _cuts_around_keys(name, n_keys=10):
    """Cut positions P - 3 .. P + 1 around candidates P of the whole buffer: keys
    straddle cuts, end exactly at a buffer's end, and leave their last 1..3
    bytes at the start of the next buffer."""
    d = _data(name)
    P = oracle.candidates(_ref(name), d).astype(np.int64)
    P = P[(P > 8) & (P < len(d) - 8)]
    assert len(P) >= n_keys
    cuts = set()
    for p in P[np.linspace(0, len(P) - 1, n_keys).astype(int)]:
        cuts.update(int(p) + k for k in range(-3, 2))
    return sorted(cuts)


@functools.lru_cache(maxsize=None)
def _key_pieces(name, n_keys=10):
    d = _data(name)
    edges = [0] + _cuts_around_keys(name, n_keys) + [len(d)]
    return tuple(d[a:b] for a, b in zip(edges[:-1], edges[1:]))


def _oracle_candidates(name, pieces):
    want = [oracle.candidates(_ref(name), p) for p in pieces]
    off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    return (np.concatenate(want) if want else np.zeros(0, np.uint64)), off


def _same_candidates(got, want):
    pos, off, allp = got
    assert not allp
    assert np.array_equal(off, want[1])
    assert np.array_equal(pos, want[0])


def _same_records(got, want):
    assert np.array_equal(got[1], want[1])
    for f in ("offset", "pool_index", "candidate"):
        assert np.array_equal(got[0][f], want[0][f]), f


@pytest.mark.parametrize("name", ["C", "short", "rx"])
def test_results_equal_the_host_batch_path(name):
    pieces = _key_pieces(name)
    assert min(len(p) for p in pieces) == 1
    sc = _scanner(name)
    src, views, host = _place(pieces, [k % 16 for k in range(len(pieces))])
    got = sc.batch_candidates_device(views)
    _same_candidates(got, sc.batch_candidates(pieces))
    _same_candidates(got, _oracle_candidates(name, pieces))
    _same_records(sc.batch_verify_calls_device(views), sc.batch_verify_calls(pieces))
    bases = np.array([k * 0x1000 + 7 for k in range(len(pieces))], np.uint64)
    _same_records(sc.batch_verify_calls_device(views, bases), sc.batch_verify_calls(pieces, bases))
    # (ptr, size) pairs are buffers too
    pairs = [(v.data_ptr() if v.numel() else 0, v.numel()) for v in views]
    _same_candidates(sc.batch_candidates_device(pairs), got[:2])
    _unchanged(src, host)


def test_bases_fixed_offset():
    """`lit` holds a string `at 4096`: its call is kept only in the buffer
    whose bases[k] + offset is 4096 (test_gpu_batch.py's test of that name)."""
    name = "lit"
    z = np.load(tables_npz(name))
    sidx = np.flatnonzero(z["str_flags"] & 0x8000)   # STRING_FLAGS_FIXED_OFFSET
    assert len(sidx) == 1 and z["str_fixed_offset"][sidx[0]] == 4096
    pool = np.flatnonzero(z["pool_string"] == sidx[0])
    d = _data(name)
    pieces = [d[:4000], d[4000:8192], d[4000:8192], d[8192:20000]]
    bases = np.array([0, 4000, 4001, 12345], np.uint64)
    sc = _scanner(name)
    src, views, host = _place(pieces, [1, 6, 11, 15])
    rec, off = sc.batch_verify_calls_device(views, bases)
    _same_records((rec, off), sc.batch_verify_calls(pieces, bases))
    per = [rec[int(off[k]):int(off[k + 1])] for k in range(4)]
    kept = [p[np.isin(p["pool_index"], pool)] for p in per]
    assert [len(k) for k in kept] == [0, 1, 0, 0] and kept[1]["offset"][0] == 96
    # without bases every buffer's base is 0: the call at local offset 96 is dropped
    rec0, off0 = sc.batch_verify_calls_device(views)
    assert not np.any(np.isin(rec0["pool_index"], pool))
    _same_records((rec0, off0), sc.batch_verify_calls(pieces))


# -- 3. many tiny buffers ------------------------------------------------------------------

def test_many_tiny_buffers():
    """70,000 buffers of 0..64 bytes at random misalignments."""
    name = "short"
    d = _data(name)
    rng = np.random.default_rng(11)
    n = 70000
    sizes = rng.integers(0, 65, n)
    begins = rng.integers(0, len(d) - 64, n)
    pieces = [d[b:b + s] for b, s in zip(begins, sizes)]
    sc = _scanner(name)
    src, views, host = _place(pieces, rng.integers(0, 16, n).tolist())
    pairs = [(v.data_ptr() if v.numel() else 0, v.numel()) for v in views]
    _same_candidates(sc.batch_candidates_device(pairs), _oracle_candidates(name, pieces))
    rec, off = sc.batch_verify_calls_device(pairs)
    assert len(off) == n + 1 and off[0] == 0 and off[-1] == len(rec)
    assert np.all(np.diff(off.astype(np.int64)) >= 0)
    sample = sorted(set(rng.integers(0, n, 150).tolist()) | {0, n - 1})
    for k in sample:
        assert np.array_equal(rec[int(off[k]):int(off[k + 1])], sc.verify_calls(pieces[k])), k
    _unchanged(src, host)


# -- 4. lifetime, 5. overflow, 6. mixing, 7. root ------------------------------------------

def test_sources_may_change_after_the_result():
    import torch
    name = "rx"
    pieces = _key_pieces(name)
    sc = _scanner(name)
    want = sc.batch_verify_calls(pieces)
    assert len(want[0]) > 0
    src, views, _ = _place(pieces, [(5 * k + 3) % 16 for k in range(len(pieces))])
    sc.scan_batch_gather_device([v.data_ptr() if v.numel() else 0 for v in views],
                                [v.numel() for v in views])
    cand = sc.batch_result()
    src.fill_(0xFF)
    torch.cuda.synchronize()
    assert int(src.min()) == 0xFF
    _same_records(sc.verify_batch_device(), want)
    _same_candidates(cand, _oracle_candidates(name, pieces))


def test_overflow_rerun_underneath():
    """A dense batch (`short` on alpha data) overflows the segments' default
    output capacity: the exact-offset rerun reads the gathered arena."""
    name = "short"
    d = _data(name)
    whole = oracle.candidates(_ref(name), d)
    assert len(whole) > 64 * (len(d) // 4096) * 2   # (test_gpu_batch.py test_overflow_rerun)
    edges = [0, 5, 70001, 70002, 200000, len(d)]
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    src, views, host = _place(pieces, [9, 4, 15, 0, 1])
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    sc = yara_amd.Scanner(tab)   # (a fresh scanner: no learned capacity)
    got = sc.batch_candidates_device(views)
    _same_candidates(got, _scanner(name).batch_candidates(pieces))
    _same_candidates(got, _oracle_candidates(name, pieces))
    _same_records(sc.batch_verify_calls_device(views), _scanner(name).batch_verify_calls(pieces))
    _unchanged(src, host)


def test_mixing_with_other_scans():
    name = "rx"
    d = _data(name)
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    sc = yara_amd.Scanner(tab)
    block = d[:100000]
    pieces = _key_pieces(name, 5)
    want_c = _oracle_candidates(name, pieces)
    want_r = _scanner(name).batch_verify_calls(pieces)
    rec0 = _scanner(name).verify_calls(block)
    src, views, _ = _place(pieces, [(k + 8) % 16 for k in range(len(pieces))])
    _same_candidates(sc.batch_candidates_device(views), want_c)
    _same_records(sc.batch_verify_calls_device(views), want_r)
    assert np.array_equal(sc.verify_calls(block), rec0)                 # a single-block scan
    _same_records(sc.batch_verify_calls(pieces), want_r)                # a host batch
    _same_records(sc.batch_verify_calls_device(views), want_r)
    assert np.array_equal(sc.candidates(block)[0], oracle.candidates(_ref(name), block))
    # a gather batch is a batch: verified by the batch call only
    sc.scan_batch_gather_device([v.data_ptr() if v.numel() else 0 for v in views],
                                [v.numel() for v in views])
    sc.batch_result()
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.verify_device()
    assert e.value.code == _lib.INVALID_ARGUMENT
    _same_records(sc.verify_batch_device(), want_r)


def test_root_accepting_tables():
    d = case_data(golden()["cases"]["root_4K"])
    tab = yara_amd.Tables.from_npz(tables_npz("root"), device=0, strings=True)
    sc = yara_amd.Scanner(tab)
    pieces = [d[:100], d[100:101], d[101:]]
    src, views, _ = _place(pieces, [3, 8, 13])
    pos, off, allp = sc.batch_candidates_device(views)
    assert allp and len(pos) == 0 and np.array_equal(off, np.zeros(4))
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.batch_verify_calls_device(views)
    assert e.value.code == _lib.INVALID_ARGUMENT
    # the single-block path still serves such rules
    assert len(sc.verify_calls(pieces[0])) > 0
