"""Pre-verification of long match lists, pinned to stock libyara.

verify.hip walks a candidate's whole match list: pass 0 decides every entry
and keeps the decisions in a 31-bit mask, pass 1 writes the records.  The
length of the list steers the code that runs:

  * up to 31 entries: pass 1 writes from the mask; a table whose longest list
    is at most 31 (and that has a "kept" 1-byte key) takes the lean write kernel
    (scanner.cpp ``direct``), which never decides;
  * 32 and more: the mask overflows and pass 1 decides every entry again;
  * "kept" 1-byte keys (up to 30 plain fits-in-atom literals): up to 4 entries
    are written from kernel arguments, 5 .. 30 by the list walk with a full
    mask, in the lean and in the persistent kernel.

Two rule sets (tests/golden/rules/lists31.yar: longest list exactly 31;
lists70.yar: lists of 32, 33 and 70, the last a chain that shares its tail
with its suffix states' lists) were compiled by the stock compiler, and a
planted buffer of each scanned by stock libyara (tests/golden/make_lists.py;
planted_lists.lists_buffer).  The CPU tests assert the list lengths from the pool
chains, pin the oracle to the recorded stock stream and match set, and count
-- from the oracle alone -- that the buffer exercises every index the kernels
treat specially.  The GPU tests compare every path's records with the oracle's
verify stream filtered by oracle.literal_effect, bit-exact and in order.
"""
import functools
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, case_arrays, ref_tables, tables_npz

SETS = ["lists31", "lists70"]
# the shortest list that fills the keep mask (lists31: bit 30 set, the lean
# kernel) / overflows it (lists70)
LONG = {"lists31": 31, "lists70": 32}

SF_NO_CASE, SF_FULL_WORD, SF_LITERAL, SF_FITS_IN_ATOM, SF_FIXED_OFFSET = 0x04, 0x80, 0x400, 0x800, 0x8000
REC_COUNT_ONLY = 0x80000000   # include/yara_amd.h YR_AMD_REC_COUNT_ONLY


def _spec(name):
    with open(os.path.join(GOLDEN, "lists.json")) as f:
        return json.load(f)["cases"]["%s_64K" % name]


@functools.lru_cache(maxsize=None)
def _tables(name):
    return dict(np.load(tables_npz(name)))


@functools.lru_cache(maxsize=None)
def _data(name):
    import planted_lists as planted
    _, _, seed, size = _spec(name)["data"]
    d = planted.lists_buffer(oracle.xorshift, name, size, seed)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _lists(name):
    """head (1-based pool index) -> the 0-based pool indices of its chain."""
    z = _tables(name)
    nx = z["pool_next"]
    out = {}
    for h in np.unique(z["M"][z["M"] != 0]).tolist():
        chain, q = [], h
        while q:
            chain.append(q - 1)
            assert len(chain) <= len(nx)
            q = int(nx[q - 1])
        out[h] = np.array(chain, np.int64)
    return out


def _oracle_stream(name, data):
    """The oracle's verify stream of `data` alone: (positions, pool indices,
    keep mask, candidate index of every call, candidate positions)."""
    ref = ref_tables(name)
    P, K = oracle.walk_verify(ref, data)
    keep = oracle.literal_effect(_tables(name), P, K, data)
    cand = oracle.candidates(ref, data)
    ci = np.searchsorted(cand, P)
    assert len(P) == 0 or np.array_equal(cand[ci], P)
    return P, K, keep, ci, cand


@functools.lru_cache(maxsize=None)
def _whole(name):
    out = _oracle_stream(name, _data(name))
    for a in out:
        a.setflags(write=False)
    return out


def _records(name, P, K, sel, ci, profile_keep=None):
    """Expected device records of the calls `sel` of a stream."""
    import yara_amd
    bt = _tables(name)["pool_backtrack"]
    out = np.zeros(int(sel.sum()), dtype=yara_amd._lib.VERIFY_REC_DTYPE)
    out["offset"] = P[sel] - bt[K[sel]].astype(np.uint64)
    out["pool_index"] = K[sel]
    if profile_keep is not None:
        out["pool_index"] |= np.where(profile_keep[sel], 0, REC_COUNT_ONLY).astype(np.uint32)
    out["candidate"] = ci[sel]
    return out


def _assert_records(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in ("offset", "pool_index", "candidate"):
        np.testing.assert_array_equal(got[f], want[f], err_msg="%s %s" % (what, f))


@functools.lru_cache(maxsize=None)
def _call_index(name):
    """Per call of the whole buffer's stream: its entry's index in its
    candidate's list (skipped entries counted, as the kernels count them) and
    the list's length; per candidate: list length, calls, kept calls, skipped
    entries."""
    z = _tables(name)
    P, K, keep, ci, cand = _whole(name)
    pos, _, match = oracle.trace(ref_tables(name), _data(name))
    head = dict(zip(pos[match != 0].tolist(), match[match != 0].tolist()))
    assert sorted(head) == cand.tolist()
    bt = z["pool_backtrack"]
    t = np.zeros(len(P), np.int64)
    length = np.zeros(len(P), np.int64)
    per = np.zeros((len(cand), 4), np.int64)
    at = 0
    for c, p in enumerate(cand.tolist()):
        chain = _lists(name)[head[p]]
        made = np.flatnonzero(bt[chain] <= p)          # scanner.c:110
        n = len(made)
        assert np.array_equal(K[at:at + n], chain[made]) and np.all(P[at:at + n] == p)
        t[at:at + n] = made
        length[at:at + n] = len(chain)
        per[c] = (len(chain), n, keep[at:at + n].sum(), len(chain) - n)
        at += n
    assert at == len(P)
    return t, length, per


# -- CPU: the fixtures hold what the GPU tests need ----------------------------------

def _kinds(name, chain):
    z = _tables(name)
    fl = z["str_flags"][z["pool_string"][chain]]
    rk = z["re_kind"][chain]
    lit = (fl & SF_LITERAL) != 0
    return dict(
        plain=int((lit & ((fl & (SF_NO_CASE | SF_FULL_WORD | SF_FITS_IN_ATOM)) == 0)).sum()),
        nocase=int((lit & ((fl & (SF_NO_CASE | SF_FITS_IN_ATOM)) == SF_NO_CASE)).sum()),
        fullword=int((lit & ((fl & (SF_FULL_WORD | SF_FITS_IN_ATOM)) == SF_FULL_WORD)).sum()),
        fast_hex=int((rk == 1).sum()), regexp=int((rk == 2).sum()),
        kept_class=int((((fl & (SF_LITERAL | SF_FITS_IN_ATOM)) == (SF_LITERAL | SF_FITS_IN_ATOM))
                        & ((fl & (SF_NO_CASE | SF_FULL_WORD | SF_FIXED_OFFSET)) == 0)).sum()),
        fits_fullword=int(((fl & (SF_FITS_IN_ATOM | SF_FULL_WORD)) == (SF_FITS_IN_ATOM | SF_FULL_WORD)).sum()))


def _split_lists(name):
    """(4-byte-atom lists, 1-byte-key lists) as lists of pool-index chains."""
    bt = _tables(name)["pool_backtrack"]
    four = [c for c in _lists(name).values() if bt[c[0]] >= 4]
    one = [c for c in _lists(name).values() if np.all(bt[c] == 1)]
    return four, one


def _mixed(name, chain):
    k = _kinds(name, chain)
    return min(k["plain"], k["nocase"], k["fullword"], k["fast_hex"], k["regexp"]) > 0


def test_lists31_table_properties():
    name = "lists31"
    four, one = _split_lists(name)
    assert max(len(c) for c in _lists(name).values()) == 31
    long4 = [c for c in four if len(c) == 31]
    assert len(long4) == 1 and _mixed(name, long4[0]), _kinds(name, long4[0])
    assert sorted(len(c) for c in one) == [4, 5, 30, 31]
    for c in one:   # every entry of the "kept" class (scanner.cpp key_classes)
        assert _kinds(name, c)["kept_class"] == len(c)


def test_lists70_table_properties():
    name = "lists70"
    z = _tables(name)
    bt = z["pool_backtrack"]
    four, one = _split_lists(name)
    sizes = sorted(len(c) for c in four)
    assert sizes.count(32) == 1 and sizes.count(33) == 1 and sizes[-1] >= 64
    for n in (32, 33, sizes[-1]):
        c = [c for c in four if len(c) == n][0]
        assert _mixed(name, c), (n, _kinds(name, c))
    # the longest list is a shared-tail chain: its last entries have smaller
    # backtracks and ARE its suffix states' lists (the same pool records)
    c = [c for c in four if len(c) == sizes[-1]][0]
    own = int((bt[c] >= 4).sum())
    assert np.all(bt[c[:own]] >= 4) and np.all(bt[c[own:]] < 4) and own > 31
    heads = {int(h) - 1: len(ch) for h, ch in _lists(name).items()}
    tails = [heads[int(q)] for q in c[1:] if int(q) in heads]
    assert len(tails) >= 2 and tails[0] == len(c) - own and tails == sorted(tails, reverse=True)
    assert len(np.unique(bt[c[own:]])) >= 2
    # entries whose atom lies behind a prefix: skipped near the buffer's start
    assert int((bt[c] > 4).sum()) >= 2
    assert sorted(len(c) for c in one) == [5, 30, 33]
    for c in one:
        k = _kinds(name, c)
        if len(c) == 33:
            assert abs(2 * k["fits_fullword"] - 33) == 1 and k["kept_class"] == 33 - k["fits_fullword"]
        else:
            assert k["kept_class"] == len(c)


@pytest.mark.parametrize("name", SETS)
def test_fixture_sizes(name):
    for f in (tables_npz(name), os.path.join(GOLDEN, "cases", "%s_64K.npz" % name)):
        assert os.path.getsize(f) <= 483175
    assert _spec(name)["size"] == (64 << 10) + 77 == len(_data(name))


@pytest.mark.parametrize("name", SETS)
def test_oracle_walk_equals_stock_verify_stream(name):
    spec, arr = _spec(name), case_arrays("%s_64K" % name)
    P, K, _, _, _ = _whole(name)
    assert spec["rc"] == 0 and len(arr["verify_pos"]) == spec["verify_count"] == len(P)
    assert oracle.verify_stream_sha(arr["verify_pos"], arr["verify_idx"]) == spec["verify_sha"]
    assert not arr["verify_base"].any()
    np.testing.assert_array_equal(P, arr["verify_pos"])
    np.testing.assert_array_equal(K, arr["verify_idx"])


@pytest.mark.parametrize("name", SETS)
def test_oracle_keeps_every_match_stock_reported(name):
    """test_preverify.py test_oracle_keeps_every_reported_match on the recorded
    stock match set of the long-list buffers."""
    import hashlib
    spec, arr, z = _spec(name), case_arrays("%s_64K" % name), _tables(name)
    mt = np.zeros(len(arr["match_string"]),
                  dtype=[("s", "<u4"), ("o", "<u8"), ("l", "<u4"), ("x", "<u4")])
    mt["s"], mt["o"], mt["l"], mt["x"] = (arr["match_string"], arr["match_offset"],
                                          arr["match_len"], arr["match_xor"])
    assert len(mt) == spec["match_count"] > 1000
    assert hashlib.sha256(mt.tobytes()).hexdigest() == spec["match_sha"]
    P, K, keep, _, _ = _whole(name)
    off = P - z["pool_backtrack"][K].astype(np.uint64)
    ps, flags = z["pool_string"], z["str_flags"]
    kept = set(zip(off[keep].tolist(), ps[K[keep]].tolist()))
    by_string = {}
    for o_, s_ in kept:
        by_string.setdefault(s_, []).append(o_)
    by_string = {k: np.sort(np.array(v, np.int64)) for k, v in by_string.items()}
    n_lit = n_re = 0
    for s, o, n in zip(mt["s"].tolist(), mt["o"].tolist(), mt["l"].tolist()):
        if flags[s] & SF_LITERAL:
            assert (o, s) in kept, (name, s, o)
            n_lit += 1
        else:
            # regexp / hex: the atom lies inside the reported match, so some
            # kept call of that string has its atom offset in [o, o + len]
            v = by_string.get(s)
            assert v is not None, (name, s, o)
            j = np.searchsorted(v, o)
            assert j < len(v) and v[j] <= o + n, (name, s, o, n)
            n_re += 1
    assert n_lit > 0 and n_re > 0 and keep.sum() < len(keep)


def _both(mask, keep):
    return int((mask & keep).sum()), int((mask & ~keep).sum())


@pytest.mark.parametrize("name", SETS)
def test_buffer_exercises_every_special_index(name):
    """Non-vacuity, from the oracle alone: kept AND dropped calls at the entry
    indices the kernels treat specially (on lists with data-dependent entries:
    the 4-byte-atom lists and lists70's half-fullword key), long lists that
    keep nothing and everything, long-list candidates sharing 64-candidate
    groups, and skipped entries at the buffer's start."""
    z = _tables(name)
    P, K, keep, ci, cand = _whole(name)
    t, length, per = _call_index(name)
    bt = z["pool_backtrack"]
    four = np.zeros(len(z["pool_next"]) + 1, bool)
    for h, c in _lists(name).items():
        four[h] = bt[c[0]] >= 4
    pos, _, match = oracle.trace(ref_tables(name), _data(name))
    call4 = four[match[np.searchsorted(pos, P)]]        # the call's list is a 4-byte atom's
    if name == "lists31":
        assert length.max() == 31
        assert min(_both((t == 30) & call4, keep)) > 0, _both((t == 30) & call4, keep)
        assert min(_both((t == 30) & ~call4, keep)) == 0    # (the 31-entry key: every call kept)
        assert int(((t == 30) & ~call4).sum()) > 0
    else:
        for sel in (t == 31, t == 32, t >= 63):
            assert min(_both(sel & call4, keep)) > 0, _both(sel & call4, keep)
        # the 33-entry key's list: all kept between non-word bytes, about half otherwise
        assert min(_both((t >= 31) & ~call4, keep)) > 0
    long_ = per[:, 0] >= LONG[name]
    assert int((long_ & (per[:, 2] == 0)).sum()) > 0
    assert int((long_ & (per[:, 2] == per[:, 0])).sum()) > 0
    assert int((long_ & (per[:, 2] > 0) & (per[:, 2] < per[:, 1])).sum()) > 100
    groups = np.bincount(np.flatnonzero(long_) // 64)
    assert int((groups >= 2).sum()) >= 8, groups
    assert len(np.unique(np.flatnonzero(long_) % 64)) == 64     # every lane
    # An entry with backtrack > position can only belong to a state as deep as
    # YR_MAX_ATOM_LENGTH (a shorter atom is a whole string: backtrack = depth,
    # atoms.c:1406-1433), so the first position with skipped entries is 4: the
    # atom at offset 0.  (Offsets 1 .. 3: the batch test's buffers.)
    early = (cand < 8) & (per[:, 3] > 0)
    assert int(early.sum()) > 0 and int(per[early, 1].min()) > 0
    if name == "lists70":   # ... and the shared-tail entries are called there
        assert int((bt[K[(P == 4)]] < 4).sum()) > 0


def _batch_edges(name):
    """Edges of at least 64 buffers cut from the planted buffer: buffers that
    begin 0 .. 3 bytes before a planted atom (entries with a larger backtrack
    are skipped there), end 0 .. 3 bytes after a planted piece, end inside an
    atom or inside the zeros after it (literal and regexp tails cut by the
    size), begin or end at a 1-byte key, and buffers of 0 and 1 bytes."""
    import planted_lists as planted
    spec = _spec(name)
    lay = planted.lists_layout(name, spec["size"], spec["data"][2])
    keys = planted.LISTS[name]["keys"]
    atoms = [x for x in lay[1:-1] if x[3] - x[2] > 1 and len(x[1]) - (x[3] - x[0]) >= 3]
    ones = [x for x in lay[1:-1] if x[3] - x[2] == 1 and x[1][x[2] - x[0]] in keys]
    atom = planted.LISTS[name]["atoms"][0]
    first = [x for x in atoms if bytes(x[1][x[2] - x[0]:x[3] - x[0]]) == atom]
    cuts = []
    pick = lambda v, n: [v[int(j)] for j in np.linspace(0, len(v) - 1, n)]   # noqa: E731
    for k, (off, piece, a, b) in enumerate(pick(first, 16)):
        cuts.append(a - k % 4)
    for k, (off, piece, a, b) in enumerate(pick(atoms, 32)):
        fam, d = divmod(k % 8, 4)
        cuts.append((off + len(piece) + d, (a + 2, b + 1, b + 2, b + 3)[d])[fam])
    for k, (off, piece, a, b) in enumerate(pick(ones, 24)):
        cuts.append((a, b, b + 1)[k % 3])
    cuts = sorted(set(c for c in cuts if 0 < c < spec["size"]))
    # empty and 1-byte buffers: an edge twice, and an edge one byte on
    extra = [cuts[5], cuts[20] + 1, cuts[40], cuts[40], spec["size"]]
    return [0] + sorted(cuts + extra) + [spec["size"]]


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(pieces, expected records, expected offsets) of the batch tests."""
    d = _data(name)
    edges = _batch_edges(name)
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    want, skipped = [], 0
    bt = _tables(name)["pool_backtrack"]
    for p in pieces:
        P, K, keep, ci, cand = _oracle_stream(name, p)
        want.append((P, K, keep, ci))
        skipped += int((bt[K].astype(np.uint64) > P).sum())
    assert skipped == 0     # (the oracle makes no call with backtrack > position)
    return pieces, want


@pytest.mark.parametrize("name", SETS)
def test_batch_buffers_cover_the_cuts(name):
    import planted_lists as planted
    pieces, want = _batch(name)
    sizes = [len(p) for p in pieces]
    assert len(pieces) >= 64 and sizes.count(0) >= 2 and sizes.count(1) >= 1
    assert sum(sizes) == len(_data(name)) and len(set(s % 16 for s in sizes)) >= 12
    # buffers beginning with an atom at offsets 0 .. 3: long lists with skipped
    # entries at positions 4 .. 7
    bt = _tables(name)["pool_backtrack"]
    longest = max(_split_lists(name)[0], key=len)
    atom = planted.LISTS[name]["atoms"][0]
    seen = set()
    for p, (P, K, keep, ci) in zip(pieces, want):
        for d in range(4):
            if bytes(p[d:d + 4]) == atom:
                made = K[P == d + 4]
                assert np.array_equal(made, longest[bt[longest] <= d + 4]) and len(made) < len(longest)
                seen.add(d)
    assert seen == {0, 1, 2, 3}
    # long lists in most buffers, kept and dropped calls overall
    n_long = sum(int(np.count_nonzero(np.bincount(ci) >= LONG[name] - 2)) for _, _, _, ci in want if len(ci))
    assert n_long > 500
    # buffers that end right after a 1-byte key and buffers that begin with one
    keys = planted.LISTS[name]["keys"]
    assert sum(len(p) > 0 and p[-1] in keys for p in pieces) >= 4
    assert sum(len(p) > 0 and p[0] in keys for p in pieces) >= 4


# -- GPU --------------------------------------------------------------------------

def _scanner(name, profiling=False):
    import yara_amd
    tab = yara_amd.Tables.from_npz(tables_npz(name), device=0, strings=True)
    if profiling:
        tab.set_profiling(True)
    return yara_amd.Scanner(tab)


def _upload(data):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(data).copy()).cuda()
    torch.cuda.synchronize()
    return d


def _device_scan(sc, run):
    """Candidates and records of one device scan started by `run`."""
    import torch
    import yara_amd
    from yara_amd._hip import d2h_u64, memcpy
    run()
    ptr, cnt, allp = sc.device_result()
    assert not allp
    p, m = sc.verify_device(0)
    rec = np.zeros(m, dtype=yara_amd._lib.VERIFY_REC_DTYPE)
    if m:
        h = torch.empty(m * 16, dtype=torch.uint8, device="cuda")
        memcpy(h.data_ptr(), p, m * 16, 3)
        rec = np.frombuffer(h.cpu().numpy().tobytes(), dtype=yara_amd._lib.VERIFY_REC_DTYPE)
    torch.cuda.synchronize()
    return d2h_u64(ptr, cnt), rec


def _range_want(name, lo, hi):
    """Candidates and records of the byte range [lo, hi) of the whole buffer:
    the positions (lo, hi] (and 0 for lo = 0), candidate fields local to it."""
    P, K, keep, ci, cand = _whole(name)
    insel = lambda x: (x <= hi) & ((x > lo) | (lo == 0))   # noqa: E731
    c = cand[insel(cand)]
    sel = keep & insel(P)
    return c, _records(name, P, K, sel, np.searchsorted(c, P))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_calls(name):
    """The verified-only host path (yr_amd_scan_block_verified)."""
    P, K, keep, ci, _ = _whole(name)
    _assert_records(_scanner(name).verify_calls(_data(name)), _records(name, P, K, keep, ci))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_full_device_scan(name):
    """A full scan of the device-resident buffer on a fresh scanner and
    yr_amd_verify_device: the candidate stream and the same records."""
    P, K, keep, ci, cand = _whole(name)
    d = _upload(_data(name))
    sc = _scanner(name)
    got_c, got = _device_scan(sc, lambda: sc.scan_device(d.data_ptr(), len(_data(name))))
    np.testing.assert_array_equal(got_c, cand)
    _assert_records(got, _records(name, P, K, keep, ci))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_profiling(name):
    """yr_amd_tables_set_profiling forces pass 1 to decide again for every
    candidate with a record: kept records unchanged, count-only records exactly
    where test_preverify.py test_profiling_count_only_records' formula says."""
    z = _tables(name)
    P, K, keep, ci, cand = _whole(name)
    n = len(_data(name))
    off = P - z["pool_backtrack"][K].astype(np.uint64)
    sf = z["str_flags"][z["pool_string"][K]]
    fixed = z["str_fixed_offset"][z["pool_string"][K]]
    counted = (off < n) & (((sf & SF_FIXED_OFFSET) == 0) | (fixed == off.astype(np.int64)))
    want = _records(name, P, K, keep | counted, ci, profile_keep=keep)
    assert np.count_nonzero(want["pool_index"] & REC_COUNT_ONLY) > 1000
    sc = _scanner(name, profiling=True)
    _assert_records(sc.verify_calls(_data(name)), want, "verified-only")
    d = _upload(_data(name))
    full = _scanner(name, profiling=True)
    got_c, got = _device_scan(full, lambda: full.scan_device(d.data_ptr(), n))
    np.testing.assert_array_equal(got_c, cand)
    _assert_records(got, want, "full scan")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_byte_ranges(name):
    """Byte-range scans [0, cut + 5) and [cut, n) with the cut inside a planted
    long-list instance (test_preverify.py
    test_verified_only_scan_keeps_records_and_candidate_indices' ranges), full
    and verified-only."""
    import planted_lists as planted
    spec = _spec(name)
    n = spec["size"]
    lay = planted.lists_layout(name, n, spec["data"][2])
    atom = planted.LISTS[name]["atoms"][0]
    # (a range begins at a multiple of 16: an instance whose atom straddles one)
    inst = [x for x in lay if bytes(x[1][x[2] - x[0]:x[3] - x[0]]) == atom and x[2] > n // 3
            and x[2] % 16 == 14]
    cut = inst[0][2] + 2       # two bytes into the atom
    assert cut % 16 == 0
    d = _upload(_data(name))
    sc = _scanner(name)
    for lo, hi in ((0, cut + 5), (cut, n)):
        want_c, want = _range_want(name, lo, hi)
        assert len(want) > 1000
        for vo in (False, True):
            sc.set_verified_only(vo)
            got_c, got = _device_scan(sc, lambda: sc.scan_device(d.data_ptr(), n, lo, hi))
            if not vo:
                np.testing.assert_array_equal(got_c, want_c)
            assert sc.stream_length() == len(want_c)
            _assert_records(got, want, "[%d, %d) verified-only=%s" % (lo, hi, vo))
    sc.set_verified_only(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_three_shards_through_windows(name):
    """Three shards, each scanned from a device window holding the shard and
    the tables' verify halos (yr_amd_scan_window): concatenated, the whole
    block's records."""
    from yara_amd import dist as ydist
    P, K, keep, ci, cand = _whole(name)
    data = _data(name)
    n = len(data)
    sc = _scanner(name)
    before, after = ydist.tables_halos(sc.tables)
    got = []
    for r in range(3):
        b, e = ydist.shard_bounds(n, 3, r, align=1 << 12)
        lo, hi = ydist.shard_window(n, b, e, before, after)
        win = _upload(data[lo:hi])
        c, rec = _device_scan(sc, lambda: sc.scan_window(win.data_ptr(), lo, hi, n, b, e))
        want_c, want_r = _range_want(name, b, e)
        np.testing.assert_array_equal(c, want_c)
        _assert_records(rec, want_r, "shard %d" % r)
        got.append(rec)
    got = np.concatenate(got)
    whole = _records(name, P, K, keep, ci)
    np.testing.assert_array_equal(got["offset"], whole["offset"])
    np.testing.assert_array_equal(got["pool_index"], whole["pool_index"])


def _batch_want(name):
    import yara_amd
    pieces, want = _batch(name)
    recs = [_records(name, P, K, keep, ci) for P, K, keep, ci in want]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    return pieces, (np.concatenate(recs) if recs else np.zeros(0, yara_amd._lib.VERIFY_REC_DTYPE)), off


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_batch_host(name):
    """yr_amd_scan_batch_verified: every buffer's records are the oracle's
    filtered stream of that slice alone (the result layout of
    test_gpu_batch.py: records[offsets[k]:offsets[k + 1]])."""
    from test_gpu_batch import _same_records
    pieces, rec, off = _batch_want(name)
    _same_records(_scanner(name).batch_verify_calls(pieces), (rec, off))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_batch_gather(name):
    """The same buffers scattered in device memory at odd addresses
    (yr_amd_scan_batch_gather_device)."""
    from test_gpu_batch import _same_records
    from test_gpu_gather import _place, _unchanged
    pieces, rec, off = _batch_want(name)
    src, views, host = _place(pieces, [(2 * k + 1) % 16 for k in range(len(pieces))])
    _same_records(_scanner(name).batch_verify_calls_device(views), (rec, off))
    _unchanged(src, host)
