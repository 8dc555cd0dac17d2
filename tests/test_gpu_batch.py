"""Batched scans on the GPU: N buffers, one scan, one pre-verification pass.

The expected result is always per buffer: oracle.candidates(ref_tables(name),
piece) for the candidate positions and the single-block Scanner.verify_calls(
piece, base) for the records.  Batches are made by cutting golden buffers.
"""
import functools

import numpy as np
import pytest

import oracle
import yara_amd
from yara_amd import _lib
from conftest import case_data, golden, ref_tables, tables_npz

pytestmark = pytest.mark.gpu

# table set -> (golden case, bytes of it used)
CASES = {
    "C": ("C_planted16M", 1 << 20),
    "lit": ("lit_1M", 1 << 20),
    "hex": ("hex_1M", 1 << 20),
    "short": ("short_1M", 1 << 18),
    "rx": ("rx_1M", 1 << 19),
    "bytekeys": ("bytekeys_1M", 1 << 18),
    "fuzz0": ("fuzz0_256K", 1 << 18),
    "fuzz3": ("fuzz3_256K", 1 << 18),
}
BYTE_KEY_SETS = ("short", "rx", "bytekeys", "fuzz0", "fuzz3")
SIZES = [0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 70001]


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
def _whole(name):
    p = oracle.candidates(_ref(name), _data(name))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _scanner(name):
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    return yara_amd.Scanner(tab)


def _cuts_around_keys(name, n_keys=10, modulo=None):
    """Cut positions P - 3 .. P + 1 around candidates P of the whole buffer: keys
    straddle cuts, end exactly at a buffer's end, and leave their last 1..3 bytes
    at the start of the next buffer.  With ``modulo`` r: only cuts congruent to
    r mod 16 (pieces then have lengths that are multiples of 16)."""
    P = _whole(name).astype(np.int64)
    n = len(_data(name))
    P = P[(P > 8) & (P < n - 8)]
    assert len(P) >= n_keys
    cuts = set()
    if modulo is None:
        for p in P[np.linspace(0, len(P) - 1, n_keys).astype(int)]:
            cuts.update(int(p) + d for d in range(-3, 2))
    else:
        # per delta, the first few candidates whose cut P + d is congruent
        for d in range(-3, 2):
            sel = P[(P + d) % 16 == modulo]
            assert len(sel) > 0
            for p in sel[np.linspace(0, len(sel) - 1, max(2, n_keys // 5)).astype(int)]:
                cuts.add(int(p) + d)
                cuts.add(int(p) + d + 16)    # a 16-byte piece behind the cut
    return sorted(cuts)


def _pieces(name, cuts, begin=0):
    d = _data(name)
    edges = [begin] + [c for c in cuts if begin < c < len(d)] + [len(d)]
    return [d[a:b] for a, b in zip(edges[:-1], edges[1:])]


def _want_candidates(name, pieces):
    want = [oracle.candidates(_ref(name), p) for p in pieces]
    off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    return (np.concatenate(want) if want else np.zeros(0, np.uint64)), off


def _want_records(name, pieces, bases=None):
    sc = _scanner(name)
    want = [sc.verify_calls(p, 0 if bases is None else int(bases[k])) for k, p in enumerate(pieces)]
    off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    return (np.concatenate(want) if want else np.zeros(0, _lib.VERIFY_REC_DTYPE)), off


def _same_candidates(got, want):
    pos, off, allp = got
    wpos, woff = want
    assert not allp
    assert np.array_equal(off, woff)
    assert np.array_equal(pos, wpos)


def _same_records(got, want):
    rec, off = got
    wrec, woff = want
    assert np.array_equal(off, woff)
    for f in ("offset", "pool_index", "candidate"):
        assert np.array_equal(rec[f], wrec[f]), f


def _device_batch(sc, arena, starts, sizes, bases=None, records=True):
    """One batch through the device API on the bytes of ``arena`` (numpy)."""
    import torch
    d = torch.from_numpy(np.array(arena, dtype=np.uint8)).cuda() if len(arena) else \
        torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 16 == 0
    sc.scan_batch_device(d.data_ptr(), len(arena), starts, sizes)
    cand = sc.batch_result()
    rec = sc.verify_batch_device(bases) if records else None
    torch.cuda.synchronize()
    return cand, rec


# -- cuts around a key's end ---------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_host_api_arbitrary_cuts(name):
    pieces = _pieces(name, _cuts_around_keys(name))
    assert min(len(p) for p in pieces) == 1
    sc = _scanner(name)
    want = _want_candidates(name, pieces)
    # (the cuts bite: a key that straddles one is a candidate of no piece; the
    # chosen candidates of the other sets may all be 1-byte keys)
    if name not in BYTE_KEY_SETS:
        assert want[1][-1] < len(_whole(name))
    _same_candidates(sc.batch_candidates(pieces), want)
    _same_records(sc.batch_verify_calls(pieces), _want_records(name, pieces))


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_api_back_to_back(name):
    """Pieces placed back to back, every length a multiple of 16: no gap
    separates a key's bytes from the next buffer's."""
    r = 5
    cuts = _cuts_around_keys(name, modulo=r)
    d = _data(name)
    end = r + (len(d) - r) // 16 * 16
    edges = [r] + [c for c in cuts if r < c < end] + [end]
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    sizes = np.array([len(p) for p in pieces], np.uint64)
    assert np.all(sizes % 16 == 0) and sizes.min() == 16
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    cand, rec = _device_batch(_scanner(name), d[r:end], starts, sizes)
    _same_candidates(cand, _want_candidates(name, pieces))
    _same_records(rec, _want_records(name, pieces))


@pytest.mark.parametrize("name", BYTE_KEY_SETS)
def test_cuts_next_to_one_byte_keys(name):
    """Cuts right after a 1-byte key and right before one: the scan's candidate
    classes are decided from the bytes beside such a key, which here belong to
    the gap or to the next buffer."""
    d = _data(name)
    ref = _ref(name)
    one = [b for b in range(256) if len(oracle.candidates(ref, np.array([b], np.uint8)))]
    assert one, "table set without 1-byte keys"
    at = np.flatnonzero(np.isin(d[8:-8], one))[:: max(1, len(d) // 4096)][:12] + 8
    cuts = sorted({int(a) for a in at} | {int(a) + 1 for a in at})
    pieces = _pieces(name, cuts)
    sc = _scanner(name)
    want = _want_candidates(name, pieces)
    # (pieces that begin with a 1-byte key: a candidate at local position 1)
    firsts = want[0][want[1][:-1][np.diff(want[1].astype(np.int64)) > 0].astype(np.int64)]
    assert np.count_nonzero(firsts == 1) >= len(at) // 2
    _same_candidates(sc.batch_candidates(pieces), want)
    _same_records(sc.batch_verify_calls(pieces), _want_records(name, pieces))


# -- sizes ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["C", "short"])
def test_sizes(name):
    d = _data(name)
    edges = np.concatenate([[0], np.cumsum(SIZES)])
    assert edges[-1] <= len(d)
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    sc = _scanner(name)
    _same_candidates(sc.batch_candidates(pieces), _want_candidates(name, pieces))
    _same_records(sc.batch_verify_calls(pieces), _want_records(name, pieces))


def test_empty_batches():
    sc = _scanner("C")
    e = np.zeros(0, np.uint8)
    for pieces in ([], [e], [e, e, e]):
        pos, off, allp = sc.batch_candidates(pieces)
        assert not allp and len(pos) == 0 and np.array_equal(off, np.zeros(len(pieces) + 1))
        rec, roff = sc.batch_verify_calls(pieces)
        assert len(rec) == 0 and np.array_equal(roff, np.zeros(len(pieces) + 1))
    # the device API: an empty batch is verified too
    cand, (rec, roff) = _device_batch(sc, e, [], [])
    assert len(cand[0]) == 0 and len(rec) == 0 and list(roff) == [0]


def test_many_tiny_buffers():
    """More than 65,536 buffers of 0..64 bytes: many per tile and per segment."""
    name = "short"
    d = _data(name)
    rng = np.random.default_rng(11)
    n = 70000
    sizes = rng.integers(0, 65, n)
    begins = rng.integers(0, len(d) - 64, n)
    pieces = [d[b:b + s] for b, s in zip(begins, sizes)]
    sc = _scanner(name)
    got = sc.batch_candidates(pieces)
    _same_candidates(got, _want_candidates(name, pieces))
    rec, off = sc.batch_verify_calls(pieces)
    assert len(off) == n + 1 and off[-1] == len(rec) and np.all(np.diff(off.astype(np.int64)) >= 0)
    # the records of a sample of the buffers against the single-block call
    # (70,000 single-block scans would take minutes), the first and last included
    sample = sorted(set(rng.integers(0, n, 150).tolist()) | {0, n - 1})
    for k in sample:
        want = sc.verify_calls(pieces[k])
        assert np.array_equal(rec[int(off[k]):int(off[k + 1])], want), k


# -- gaps, bases, root, overflow, mixing -------------------------------------------

@pytest.mark.parametrize("name", ["C", "short", "rx"])
def test_gap_independence(name):
    """The device API takes whatever the caller left in the gaps: zeroed gaps
    and gaps holding the key bytes before each cut give the same results."""
    d = _data(name)
    cuts = _cuts_around_keys(name)
    edges = [0] + cuts + [len(d)]
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    sizes = np.array([len(p) for p in pieces], np.uint64)
    # gaps of 16..47 bytes before every buffer
    starts, at = [], 32
    for s in sizes:
        starts.append(at)
        at = (at + int(s) + 15) // 16 * 16 + 32
    starts = np.array(starts, np.uint64)
    results = []
    for fill in (False, True):
        arena = np.zeros(at, np.uint8)
        if fill:
            # every gap ends with the bytes that precede the cut in the uncut
            # buffer (so keys straddle into the buffer exactly as there), the
            # rest holds a 1-byte-dense pattern
            arena[:] = np.resize(d[:4096], at)
        for k, p in enumerate(pieces):
            a = int(starts[k])
            if fill:
                pre = d[max(0, edges[k] - 16):edges[k]]
                arena[a - len(pre):a] = pre
            arena[a:a + len(p)] = p
        results.append(_device_batch(_scanner(name), arena, starts, sizes))
    want_c, want_r = _want_candidates(name, pieces), _want_records(name, pieces)
    for cand, rec in results:
        _same_candidates(cand, want_c)
        _same_records(rec, want_r)


def _bases_both_apis(name, pieces, bases):
    sc = _scanner(name)
    want = _want_records(name, pieces, bases)
    got = sc.batch_verify_calls(pieces, bases)
    _same_records(got, want)
    sizes = np.array([len(p) for p in pieces], np.uint64)
    starts, arena_size = yara_amd.batch_layout(sizes)
    arena = np.zeros(arena_size, np.uint8)
    for s, p in zip(starts, pieces):
        arena[int(s):int(s) + len(p)] = p
    _same_records(_device_batch(sc, arena, starts, sizes, bases)[1], want)
    return got


def test_bases_fixed_offset():
    """`lit` holds a string `at 4096`: its call is kept only in the buffer
    whose bases[k] + offset is 4096."""
    name = "lit"
    z = np.load(tables_npz(name))
    sidx = np.flatnonzero(z["str_flags"] & 0x8000)   # STRING_FLAGS_FIXED_OFFSET
    assert len(sidx) == 1 and z["str_fixed_offset"][sidx[0]] == 4096
    pool = np.flatnonzero(z["pool_string"] == sidx[0])
    d = _data(name)
    whole = _scanner(name).verify_calls(d[:20000])
    hit = whole[np.isin(whole["pool_index"], pool)]
    assert list(hit["offset"]) == [4096]   # (the golden buffer plants it there)
    pieces = [d[:4000], d[4000:8192], d[4000:8192], d[8192:20000]]
    bases = np.array([0, 4000, 4001, 12345], np.uint64)
    rec, off = _bases_both_apis(name, pieces, bases)
    per = [rec[int(off[k]):int(off[k + 1])] for k in range(4)]
    kept = [p[np.isin(p["pool_index"], pool)] for p in per]
    assert [len(k) for k in kept] == [0, 1, 0, 0] and kept[1]["offset"][0] == 96
    # without bases every buffer's base is 0: the call at local offset 96 is dropped
    rec0, off0 = _scanner(name).batch_verify_calls(pieces)
    assert not np.any(np.isin(rec0["pool_index"], pool))
    _same_records((rec0, off0), _want_records(name, pieces))


@pytest.mark.parametrize("name", ["fuzz0", "fuzz3"])
def test_bases(name):
    pieces = _pieces(name, _cuts_around_keys(name, n_keys=6))
    bases = np.array([(k * 0x1000 + 7) for k in range(len(pieces))], np.uint64)
    _bases_both_apis(name, pieces, bases)


def test_root_accepting_tables():
    d = case_data(golden()["cases"]["root_4K"])
    tab = yara_amd.Tables.from_npz(tables_npz("root"), device=0, strings=True)
    sc = yara_amd.Scanner(tab)
    pieces = [d[:100], d[100:101], d[101:]]
    pos, off, allp = sc.batch_candidates(pieces)
    assert allp and len(pos) == 0 and np.array_equal(off, np.zeros(4))
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.batch_verify_calls(pieces)
    assert e.value.code == _lib.INVALID_ARGUMENT
    import torch
    t = torch.from_numpy(d.copy()).cuda()
    sc.scan_batch_device(t.data_ptr(), 4096, [0, 112], [100, 50])
    assert sc.batch_result()[2]
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.verify_batch_device()
    assert e.value.code == _lib.INVALID_ARGUMENT
    # the single-block path still serves such rules
    assert len(sc.verify_calls(pieces[0])) > 0


def test_overflow_rerun():
    """A dense batch (`short` on alpha data) overflows the segments' default
    output capacity: the exact-offset rerun runs underneath the batch result."""
    name = "short"
    d = _data(name)
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    sc = yara_amd.Scanner(tab)   # (a fresh scanner: no learned capacity)
    # (4 KiB segments of 64 entries each at this size: the average segment overflows)
    assert len(_whole(name)) > 64 * (len(d) // 4096) * 2
    edges = [0, 5, 70001, 70002, 200000, len(d)]
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    _same_candidates(sc.batch_candidates(pieces), _want_candidates(name, pieces))
    _same_records(sc.batch_verify_calls(pieces), _want_records(name, pieces))


def test_mixing_with_single_block_scans():
    name = "rx"
    d = _data(name)
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    sc = yara_amd.Scanner(tab)
    block = d[:100000]
    pos0, _ = sc.candidates(block)
    rec0 = sc.verify_calls(block)
    assert np.array_equal(pos0, oracle.candidates(_ref(name), block))
    pieces = _pieces(name, _cuts_around_keys(name, n_keys=5))
    want_c, want_r = _want_candidates(name, pieces), _want_records(name, pieces)
    _same_candidates(sc.batch_candidates(pieces), want_c)
    _same_records(sc.batch_verify_calls(pieces), want_r)
    assert np.array_equal(sc.candidates(block)[0], pos0)
    assert np.array_equal(sc.verify_calls(block), rec0)
    _same_records(sc.batch_verify_calls(pieces), want_r)

    # cross-use: a batch scan is verified by the batch call only, a
    # single-block scan by the single-block call only
    import torch
    t = torch.from_numpy(block.copy()).cuda()
    sc.scan_batch_device(t.data_ptr(), len(block), [0, 4096], [4000, 5000])
    sc.batch_result()
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.verify_device()
    assert e.value.code == _lib.INVALID_ARGUMENT
    sc.verify_batch_device()
    sc.scan_device(t.data_ptr(), len(block))
    sc.device_result()
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.verify_batch_device()
    assert e.value.code == _lib.INVALID_ARGUMENT
    assert sc.verify_device()[1] == len(rec0)
    torch.cuda.synchronize()


def test_verified_only_has_no_effect():
    name = "fuzz3"
    pieces = _pieces(name, _cuts_around_keys(name, n_keys=5))
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    sc = yara_amd.Scanner(tab)
    sc.set_verified_only(True)
    _same_candidates(sc.batch_candidates(pieces), _want_candidates(name, pieces))
    _same_records(sc.batch_verify_calls(pieces), _want_records(name, pieces))


def test_device_api_rejects_bad_layouts():
    import torch
    sc = _scanner("C")
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for starts, sizes, ptr, size in (
            ([0, 8], [4, 4], p, 4096),         # start not 16-byte aligned
            ([16, 0], [4, 4], p, 4096),        # not ascending
            ([0, 16], [17, 4], p, 4096),       # overlap
            ([0, 4080], [4, 17], p, 4096),     # past the arena
            ([0], [4], p + 8, 4000),           # arena not aligned
            ([0], [4], p, 1 << 32)):           # arena_size + 1 > YR_AMD_VERIFY_MAX_CANDIDATES
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.scan_batch_device(ptr, size, starts, sizes)
        assert e.value.code == _lib.INVALID_ARGUMENT
