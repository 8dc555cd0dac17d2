"""The drain's other-role probe and the first level at the flush.

The pair filter holds every key window in both roles (tables.cpp filter_set:
filter_probe_left and filter_probe_right).  Stage 1 and the drain's re-test
probe a position in the role its parity gives it; on tables without 1- or
2-byte keys the product kernel's drain (kernels.hip drain, other_role_pass)
then probes the same window in the OTHER role, and only positions that pass
both go to the pending list, where flush_pending runs the first level and the
bucket probes.  A key window passes both roles by construction, so the
candidate stream is unchanged: every case here compares with
oracle.candidates(ref_tables(rules), data).

The first test needs no GPU: it pins the invariant the kernel relies on, on a
filter rebuilt from T and M the way tools/filter_model.py does.  The GPU cases
aim at what moved: positions rejected by the other role (both parities), a
drain with far more than 64 survivors (the pending list's rounds, a flush
whose lanes all pass the first level, a flush whose lanes all fail it), a
final drain that leaves the pending list empty, survivors in the ragged tail
tile, and windows that need the ring entry's context bytes (lane bytes 0 and
1) at lane, tile and segment edges.  `lit` has 2-byte keys, so its drains keep
the other path (every hit goes to the buckets); it runs the same cases.
"""
import glob
import os
import sys

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, REPO, ref_tables, tables_npz

sys.path.insert(0, os.path.join(REPO, "tools"))
import filter_model as fm   # noqa: E402  (the CPU model of the filter)

TILE = 1024
SEG = 4 * TILE   # segments of small blocks (scanner.cpp choose_seg_bytes: 4 tiles at least)
_KEYS = {}
_FILTER = {}


def keys(rules):
    """{length: sorted little-endian keys} of a golden rule set (shared)."""
    if rules not in _KEYS:
        z = np.load(tables_npz(rules))
        _KEYS[rules] = {n: sorted(s) for n, s in fm.keys_of(z["T"], z["M"]).items()}
    return _KEYS[rules]


def filter_windows(k):
    """The 3-byte windows tables.cpp puts into the pair filter: a 4-byte key's
    last three bytes, a 3-byte key, a shorter key behind every leading byte."""
    w = {x >> 8 for x in k[4]} | set(k[3])
    for x in k[2]:
        w |= {lead | (x << 8) for lead in range(256)}
    out = np.array(sorted(w), np.int64)
    if k[1]:
        lead = np.arange(65536, dtype=np.int64)
        out = np.unique(np.concatenate([out] + [lead | (x << 16) for x in k[1]]))
    return out


def pair_filter(rules):
    if rules not in _FILTER:
        _FILTER[rules] = fm.build("pair", filter_windows(keys(rules)))
    return _FILTER[rules]


def role_passes(rules, data):
    """(own, other): per byte index i, the filter result of the window ending
    at byte i in the role its parity gives it (even: left) and in the other
    one; bytes before the block are zeros, as in the kernel."""
    d = np.concatenate([np.zeros(2, np.int64), data.astype(np.int64)])
    w = d[:-2] | (d[1:-1] << 8) | (d[2:] << 16)
    par = np.arange(w.size) & 1
    f = pair_filter(rules)
    own = np.where(par == 0, fm.test("pair", f, w, 0), fm.test("pair", f, w, 1))
    other = np.where(par == 0, fm.test("pair", f, w, 1), fm.test("pair", f, w, 0))
    return own.astype(bool), other.astype(bool)


def key_bytes(k, n):
    return np.frombuffer(int(k).to_bytes(n, "little"), np.uint8)


@pytest.mark.parametrize("rules", ["A", "C", "fuzz4", "lit", "fuzz5", "fuzz7"])
def test_key_windows_pass_both_roles(rules):
    """Every window of the pair filter passes filter_probe_left AND
    filter_probe_right -- for the sets without 1- or 2-byte keys (C; A and
    fuzz4 when the pair filter is forced on them) these are the 3-byte key windows
    the drain's other-role probe must never reject; for sets with 2-byte keys
    (lit, fuzz5, fuzz7), which keep the old drain, the same holds of their
    expanded windows."""
    k = keys(rules)
    W = filter_windows(k)
    assert W.size > 0
    f = pair_filter(rules)
    assert (fm.test("pair", f, W, 0) == 1).all()
    assert (fm.test("pair", f, W, 1) == 1).all()
    if not k[1] and not k[2]:
        assert W.size == len({x >> 8 for x in k[4]} | set(k[3]))


def test_dual_role_rate_of_the_model():
    """tools/filter_model.py's dual-role figures on 1 MiB: passing both roles
    is rarer than passing one, and no key window is lost."""
    r = fm.dual_role_rates(np.load(tables_npz("C")), 1)
    assert r["both_roles_pass"] < 0.5 * r["own_role_pass"]
    assert r["inherent_window_rate"] <= r["both_roles_pass"]


# --------------------------------------------------------------------------
# GPU cases
# --------------------------------------------------------------------------
_SCANNERS = {}


def scanner(rules):
    import yara_amd
    if rules not in _SCANNERS:
        t = yara_amd.Tables.from_npz(tables_npz(rules), device=0)
        if rules == "C":
            assert t.info()["filter_mode"] == 0, "the pair filter"
        _SCANNERS[rules] = (t, yara_amd.Scanner(t))
    return _SCANNERS[rules][1]


def check(rules, data, min_candidates=0):
    data = np.ascontiguousarray(data, np.uint8)
    ref = oracle.candidates(ref_tables(rules), data)
    assert len(ref) >= min_candidates
    pos, allp = scanner(rules).candidates(data)
    assert not allp
    np.testing.assert_array_equal(pos, ref)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("rules", ["C", "lit"])
@pytest.mark.parametrize("shift", [0, 1])
def test_other_role_rejections(rules, shift):
    """256 KiB of random input, and the same bytes one byte later: every window
    is seen in both parities, so each role is the re-test's for one buffer and
    the other-role probe's for the other."""
    data = oracle.xorshift((256 << 10) + 1, 7)[shift:shift + (256 << 10)]
    if rules == "C":
        own, other = role_passes(rules, data)
        print("own-role passes %d, both roles %d" % (own.sum(), (own & other).sum()))
        assert (own & ~other).sum() > 100   # positions the other role rejects
    check(rules, data)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [3, 4])
def test_pending_list_in_rounds(length):
    """One of C's keys repeated back to back over 64 KiB: nearly every lane of a
    drain holds several dual-role survivors that are keys, so one drain fills the
    pending list many times over and every lane of a flush passes the first level."""
    k = keys("C")[length][len(keys("C")[length]) // 2]
    data = np.tile(key_bytes(k, length), (64 << 10) // length + 1)[:64 << 10]
    check("C", data, min_candidates=(64 << 10) // length - 8)


@pytest.mark.gpu
def test_flush_rejects_true_windows_that_are_no_keys():
    """The last three bytes of 4-byte keys behind a wrong first byte, back to
    back: true key windows (both roles pass), hundreds per drain, that the
    first level or the buckets reject at the flush."""
    k3 = set(keys("C")[3])
    k4 = [k for k in keys("C")[4] if (k >> 8) not in k3][:4096]
    quads = np.array([(k & ~0xFF) | ((k ^ 0x55) & 0xFF) for k in k4], np.uint32)
    data = np.tile(quads.view(np.uint8), 4)[:64 << 10]
    own, other = role_passes("C", data)
    assert (own & other).sum() >= data.size // 4 - 1
    ref = check("C", data)
    print("planted %d, candidates %d" % (data.size // 4, len(ref)))
    assert len(ref) < data.size // 16


def no_dual_pass_buffer(rules, n, seed):
    """n random bytes changed until no position passes both roles, with
    positions left that pass their own."""
    data = oracle.xorshift(n, seed).copy()
    rng = np.random.default_rng(seed)
    for _ in range(200):
        own, other = role_passes(rules, data)
        bad = np.flatnonzero(own & other)
        if bad.size == 0:
            break
        data[bad] = rng.integers(0, 256, bad.size, dtype=np.uint8)
    assert bad.size == 0
    return data, int(own.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [4, 5, 6, 7])
def test_final_drain_leaves_nothing_pending(tiles):
    """Hits of the own role only: every drain, the segment's last one included,
    appends nothing, and the segment ends with an empty pending list."""
    data, own = no_dual_pass_buffer("C", tiles * TILE, 50 + tiles)
    assert own > 0
    assert len(check("C", data)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 3, 15, 17])
@pytest.mark.parametrize("k", [4, 6])
def test_last_survivor_in_the_ragged_tail(k, r):
    """A block of k tiles and r bytes whose last candidate ends at its last
    byte, in the ragged tail tile; k = 4: the tail is a segment of its own."""
    n = k * TILE + r
    data = oracle.xorshift(n, 60 + r).copy()
    key = key_bytes(keys("C")[4][17 * r], 4)
    m = min(4, n)
    data[n - m:] = key[4 - m:]
    ref = check("C", data, min_candidates=1)
    assert int(ref[-1]) == n


EDGES = [5 * 16, TILE, 3 * TILE + 16, SEG, 2 * SEG]   # a lane, tile and segment starts


@pytest.mark.gpu
@pytest.mark.parametrize("length", [3, 4])
@pytest.mark.parametrize("lane_byte", [0, 1, 14, 15])
def test_keys_ending_next_to_lane_edges(length, lane_byte):
    """Keys whose last byte is lane byte 0, 1, 14 or 15 of a lane at the start
    of a lane, a tile and a segment (lane bytes 0 and 1: the key straddles the
    edge and its window lies in the entry's context bytes), and of the lane
    before each of them (14, 15)."""
    ks = keys("C")[length]
    data = oracle.xorshift(3 * SEG, 70 + lane_byte).copy()
    ends = []
    for i, edge in enumerate(EDGES):
        lane0 = edge if lane_byte < 2 else edge - 16
        end = lane0 + lane_byte   # byte index of the key's last byte
        data[end - length + 1:end + 1] = key_bytes(ks[(97 * i + lane_byte) % len(ks)], length)
        ends.append(end + 1)
    ref = check("C", data, min_candidates=len(ends))
    assert set(ends) <= set(int(x) for x in ref)
