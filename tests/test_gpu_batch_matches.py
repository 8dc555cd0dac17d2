"""GPU: the match stage of a batch (yr_amd_match_batch_device).  Buffer k of a
batch must get exactly what the single-block call gives for that buffer alone
(Scanner.string_matches), which test_gpu_matches.py pins to stock libyara's
match lists; here the batch is pinned to both, to the rule restated in numpy
over the batch's own records, and the sort's third field -- the buffer -- is
walked through its pass counts (none, one, two, three).  Every comparison is
exact equality."""
import numpy as np
import pytest

import oracle
import yara_amd
from yara_amd import _lib
from conftest import case_data, golden, ref_tables, tables_npz
from test_gpu_parity import blocks
from test_match_abi import final_rule
import test_gpu_batch as tb
import test_gpu_matches as tm

pytestmark = pytest.mark.gpu

CASES = golden()["cases"]
INV = yara_amd.INVALID_ARGUMENT
MATCH_FIELDS = ("string", "offset", "length", "xor_key", "pool_index")
REST_FIELDS = ("offset", "pool_index", "candidate")
SETS = ["C", "lit", "short", "fuzz0", "fuzz3", "hex"]


def _off(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)


def _cat(parts, dtype):
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def singles(sc, pieces, bases=None):
    """What the batch must give: the single-block call per buffer, concatenated."""
    m, r = [], []
    for k, p in enumerate(pieces):
        a, b = sc.string_matches(p, 0 if bases is None else int(bases[k]))
        m.append(a)
        r.append(b)
    return _cat(m, _lib.MATCH_REC_DTYPE), _off(m), _cat(r, _lib.VERIFY_REC_DTYPE), _off(r)


def same(got, want, match_fields=MATCH_FIELDS):
    gm, gmo, gr, gro = got
    wm, wmo, wr, wro = want
    np.testing.assert_array_equal(gmo, wmo, err_msg="match_off")
    np.testing.assert_array_equal(gro, wro, err_msg="rest_off")
    assert gmo.dtype == np.uint64 and gro.dtype == np.uint64
    assert gm.dtype == np.dtype(_lib.MATCH_REC_DTYPE) and gr.dtype == np.dtype(_lib.VERIFY_REC_DTYPE)
    tm.assert_fields(gm, wm, match_fields)
    tm.assert_fields(gr, wr, REST_FIELDS)


def restate_batch(rules, recs, rec_off):
    """tm.restate per buffer, vectorised: (matches' string, offset, pool_index;
    match_off; rest; rest_off) of a batch's records and their CSR."""
    z = tm.npz(rules)
    n = len(rec_off) - 1
    buf = np.repeat(np.arange(n, dtype=np.int64), np.diff(rec_off.astype(np.int64)))
    string = z["pool_string"][recs["pool_index"]] if recs.size else np.zeros(0, np.uint32)
    fin = final_rule(z["str_flags"])[string] if recs.size else np.zeros(0, bool)
    rest, rest_buf = recs[~fin], buf[~fin]
    m, s, b = recs[fin], string[fin], buf[fin]
    # stable: equal (buffer, string, offset) stay in record order, the first wins
    order = np.lexsort((m["offset"], s, b))
    m, s, b = m[order], s[order], b[order]
    keep = np.ones(m.size, bool)
    keep[1:] = (b[1:] != b[:-1]) | (s[1:] != s[:-1]) | (m["offset"][1:] != m["offset"][:-1])
    out = np.zeros(int(keep.sum()), dtype=_lib.MATCH_REC_DTYPE)
    out["string"], out["offset"], out["pool_index"] = s[keep], m["offset"][keep], m["pool_index"][keep]
    edges = np.arange(n + 1)
    return (out, np.searchsorted(b[keep], edges).astype(np.uint64), rest,
            np.searchsorted(rest_buf, edges).astype(np.uint64))


def restate_loop(rules, recs, rec_off):
    """The same through tm.restate itself, one buffer at a time."""
    m, r = [], []
    for k in range(len(rec_off) - 1):
        a, b = tm.restate(rules, recs[int(rec_off[k]):int(rec_off[k + 1])])
        o = np.zeros(len(a["string"]), dtype=_lib.MATCH_REC_DTYPE)
        o["string"], o["offset"], o["pool_index"] = a["string"], a["offset"], a["pool_index"]
        m.append(o)
        r.append(b)
    return _cat(m, _lib.MATCH_REC_DTYPE), _off(m), _cat(r, _lib.VERIFY_REC_DTYPE), _off(r)


RESTATED = ("string", "offset", "pool_index")


# -- 1. per-buffer parity ------------------------------------------------------
def _gap_arena(name, pieces, edges):
    """test_gpu_batch.test_gap_independence's layout: gaps of 16..47 bytes
    before every buffer, ending with the key bytes that precede the cut."""
    d = tb._data(name)
    sizes = np.array([len(p) for p in pieces], np.uint64)
    starts, at = [], 32
    for s in sizes:
        starts.append(at)
        at = (at + int(s) + 15) // 16 * 16 + 32
    arena = np.resize(d[:4096], at).copy()
    for k, p in enumerate(pieces):
        a = starts[k]
        pre = d[max(0, edges[k] - 16):edges[k]]
        arena[a - len(pre):a] = pre
        arena[a:a + len(p)] = p
    return arena, np.array(starts, np.uint64), sizes


@pytest.mark.parametrize("name", SETS)
def test_per_buffer_parity(name):
    import torch
    d = tb._data(name)
    cuts = tb._cuts_around_keys(name)
    edges = [0] + cuts + [len(d)]
    pieces = [d[a:b] for a, b in zip(edges[:-1], edges[1:])]
    assert min(len(p) for p in pieces) == 1
    sc = tb._scanner(name)
    arena, starts, sizes = _gap_arena(name, pieces, edges)
    dev = torch.from_numpy(arena).cuda()
    assert dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    some = 0
    for bases in (None, np.array([k * 0x1000 + 7 for k in range(len(pieces))], np.uint64)):
        want = singles(sc, pieces, bases)
        some += len(want[0])
        same(sc.batch_string_matches(pieces, bases), want)
        sc.scan_batch_device(dev.data_ptr(), len(arena), starts, sizes)
        sc.batch_result()
        same(sc.match_batch_device(bases), want)
    if name != "hex":   # (hex: its literal strings are chain parts -- all rest)
        assert some > 0
    torch.cuda.synchronize()


# -- 2. stock libyara: overlapping blocks as one batch ---------------------------
@pytest.mark.parametrize("case", tm.BLOCKS)
def test_overlapping_blocks_in_one_batch(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = yara_amd.Scanner(tm.str_tables(rec["rules"]))
    cut = list(blocks(data.size, rec["block"], rec["overlap"]))
    assert len(cut) > 1
    bases = np.array([b for b, _ in cut], np.uint64)
    m, mo, _, _ = sc.batch_string_matches([data[b:b + n] for b, n in cut], bases)
    per = [(int(b), m[int(mo[k]):int(mo[k + 1])]) for k, (b, _) in enumerate(cut)]
    tm.assert_fields(yara_amd.merge_matches(per), tm.golden_matches(case, rec["rules"]))


# -- 3. whole goldens ----------------------------------------------------------
@pytest.mark.parametrize("case", tm.WHOLE)
def test_whole_goldens(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = yara_amd.Scanner(tm.str_tables(rec["rules"]))
    batch = [data[:0], data, data[:1000]]
    if case == "root_4K":   # root-accepting rules: such buffers are scanned one by one
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.batch_string_matches(batch)
        assert e.value.code == INV
        tm.assert_fields(sc.string_matches(data)[0], tm.golden_matches(case, rec["rules"]))
        return
    m, mo, r, ro = sc.batch_string_matches(batch)
    assert mo[0] == mo[1] == 0 and ro[0] == ro[1] == 0
    tm.assert_fields(m[int(mo[1]):int(mo[2])], tm.golden_matches(case, rec["rules"]))
    same((m, mo, r, ro), singles(sc, batch))


# -- 4. equal (string, offset) in different buffers are different matches --------
def test_no_merging_across_buffers():
    data = case_data(CASES["lit_1M"])
    p, q = data[:300000], data[:200001]
    sc = yara_amd.Scanner(tm.str_tables("lit"))
    mp, mq = sc.string_matches(p)[0], sc.string_matches(q)[0]
    assert len(mp) > 10 and len(mq) > 10
    m, mo, _, _ = sc.batch_string_matches([p, p, q, p])
    assert len(m) == 3 * len(mp) + len(mq) == int(mo[4])
    for k, want in enumerate((mp, mp, mq, mp)):
        tm.assert_fields(m[int(mo[k]):int(mo[k + 1])], want, MATCH_FIELDS)


# -- 5. the first call wins, across a real duplicate -----------------------------
DUP = "lists31_dup"   # lists31 with its four byte-identical "~" strings made ONE string
DUP_POOL = [52, 51, 50, 49]   # the "~" key's match list, in list order
DUP_STRING = 31


def test_first_call_wins(tmp_path):
    z = dict(np.load(tables_npz("lists31")))
    assert list(z["pool_string"][49:53]) == [31, 32, 33, 34]
    assert list(z["pool_backtrack"][49:53]) == [1, 1, 1, 1]
    assert final_rule(z["str_flags"])[31:35].all()
    z["pool_string"] = z["pool_string"].copy()
    z["pool_string"][49:53] = DUP_STRING
    path = str(tmp_path / "lists31_dup.npz")
    np.savez(path, **z)
    tm._NPZ[DUP] = z   # (what tm.restate reads for this name)
    sc = yara_amd.Scanner(yara_amd.Tables.from_npz(path, device=0, strings=True))
    buffers = [np.frombuffer(b, np.uint8) for b in (
        b"~ab~cd~~ Zq9#\x00A ~",
        b"~",
        b"~~" + b"ab~cd~~ Zq9#\x00A ~" * 5 + b"x~")]
    ref = ref_tables("lists31")   # (the automaton is the same: only the pool's strings differ)
    for b in buffers:
        # the input has the groups: every "~" gives four kept calls of one (string, offset)
        pos, idx = oracle.walk_verify(ref, b)
        keep = oracle.literal_effect(z, pos, idx, b)
        sel = keep & np.isin(idx, DUP_POOL)
        at = np.flatnonzero(b == ord("~"))
        assert len(at) >= 1 and b[0] == ord("~") and b[-1] == ord("~")
        off = pos[sel].astype(np.int64) - z["pool_backtrack"][idx[sel]].astype(np.int64)
        assert list(off) == list(np.repeat(at, 4))
        assert list(idx[sel]) == DUP_POOL * len(at)
    got = sc.batch_string_matches(buffers)
    m, mo, _, _ = got
    for k, b in enumerate(buffers):
        mk = m[int(mo[k]):int(mo[k + 1])]
        mk = mk[mk["string"] == DUP_STRING]
        assert list(mk["offset"]) == list(np.flatnonzero(b == ord("~")))
        assert np.all(mk["pool_index"] == 52) and np.all(mk["length"] == 1)
    same(got, singles(sc, buffers))
    recs, rec_off = sc.batch_verify_calls(buffers)
    assert len(recs) > len(m) + len(got[2])   # (duplicates were dropped)
    same(got, restate_loop(DUP, recs, rec_off), RESTATED)
    same(got, restate_batch(DUP, recs, rec_off), RESTATED)


# -- 6. wave, tile and buffer edges ----------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_wave_tile_and_buffer_edges(reverse):
    e = tm.edge_prefixes()
    counts = sorted(k for k in e if k != "data")
    assert counts[:-1] == tm.EDGE_COUNTS and counts[-1] > 19000
    order = counts[::-1] if reverse else counts
    pieces = [e["data"][:e[c]] for c in order]
    sc = yara_amd.Scanner(tm.str_tables("short"))
    recs, rec_off = sc.batch_verify_calls(pieces)
    assert list(np.diff(rec_off.astype(np.int64))) == order
    got = sc.batch_string_matches(pieces)
    want = restate_loop("short", recs, rec_off)
    same(got, want, RESTATED)
    same(restate_batch("short", recs, rec_off), want, RESTATED)   # (the vectorised form agrees)
    same(got, singles(sc, pieces))


# -- 7. many buffers: the sort's buffer passes -------------------------------------
def test_4096_small_buffers():
    """12 buffer bits: one full pass and one partial."""
    d = tb._data("short")
    rng = np.random.default_rng(5)
    n = 4096
    sizes = rng.integers(0, 49, n)
    for a in (0, 700, 701, n - 3):   # runs of empty buffers, at both ends too
        sizes[a:a + 3] = 0
    sizes[1000:1100] = 0
    begins = rng.integers(0, len(d) - 48, n)
    pieces = [d[b:b + s] for b, s in zip(begins, sizes)]
    sc = tb._scanner("short")
    got = sc.batch_string_matches(pieces)
    assert len(got[0]) > 1000
    same(got, singles(sc, pieces))


def test_65537_buffers():
    """17 buffer bits: three buffer passes."""
    d = tb._data("short")
    rng = np.random.default_rng(6)
    n = 65537
    begins = rng.integers(0, len(d) - 16, n)
    pieces = [d[b:b + 16] for b in begins]
    sc = tb._scanner("short")
    got = sc.batch_string_matches(pieces)
    recs, rec_off = sc.batch_verify_calls(pieces)
    assert len(got[0]) > 1000
    same(got, restate_batch("short", recs, rec_off), RESTATED)
    m, mo, r, ro = got
    sample = sorted(set(rng.integers(0, n, 150).tolist()) | {0, n - 1})
    for k in sample:
        wm, wr = sc.string_matches(pieces[k])
        np.testing.assert_array_equal(m[int(mo[k]):int(mo[k + 1])], wm, err_msg=str(k))
        np.testing.assert_array_equal(r[int(ro[k]):int(ro[k + 1])], wr, err_msg=str(k))


def test_one_buffer_and_empty_batches():
    d = tb._data("short")[:50000]
    sc = tb._scanner("short")
    got = sc.batch_string_matches([d])   # n == 1: no buffer pass
    assert len(got[0]) > 100
    same(got, singles(sc, [d]))
    e = np.zeros(0, np.uint8)
    for pieces in ([], [e, e, e]):
        m, mo, r, ro = sc.batch_string_matches(pieces)
        assert len(m) == 0 and len(r) == 0
        assert np.array_equal(mo, np.zeros(len(pieces) + 1)) and mo.dtype == np.uint64
        assert np.array_equal(ro, np.zeros(len(pieces) + 1)) and ro.dtype == np.uint64
        assert m.dtype == np.dtype(_lib.MATCH_REC_DTYPE) and r.dtype == np.dtype(_lib.VERIFY_REC_DTYPE)
        m, mo, r, ro = sc.batch_string_matches_device([])
        assert len(m) == 0 and len(r) == 0 and list(mo) == [0] and list(ro) == [0]


# -- 8. buffers scattered in device memory -----------------------------------------
def test_gather_path():
    import torch
    from test_gpu_gather import _place
    name = "lit"
    pieces = tb._pieces(name, tb._cuts_around_keys(name, n_keys=6))
    mis = [(7 * k + 1) % 16 | 1 for k in range(len(pieces))]   # odd byte offsets
    src, views, host = _place(pieces, mis)
    sc = tb._scanner(name)
    bases = np.array([k * 0x1000 + 7 for k in range(len(pieces))], np.uint64)
    for b in (None, bases):
        want = sc.batch_string_matches(pieces, b)
        assert len(want[0]) > 10
        same(sc.batch_string_matches_device(views, b), want)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), host)


# -- 9. misuse -------------------------------------------------------------------
def _refused(call):
    with pytest.raises(yara_amd.YaraAmdError) as e:
        call()
    assert e.value.code == INV


def test_misuse():
    import torch
    data = case_data(CASES["lit_1M"])[:1 << 18]
    pieces = [data[:70000], data[70000:150001]]
    sc = yara_amd.Scanner(tm.str_tables("lit"))
    _refused(sc.match_batch_device)                     # before any scan
    block_want, _ = sc.string_matches(data)             # a single-block scan
    assert len(block_want) > 10
    _refused(sc.match_batch_device)
    want = singles(sc, pieces)
    d = torch.from_numpy(data.copy()).cuda()
    torch.cuda.synchronize()
    starts, sizes = [0, 70000], [70000, 80001]
    assert starts[1] % 16 == 0
    sc.scan_batch_device(d.data_ptr(), data.size, starts, sizes)
    _refused(sc.match_batch_device)                     # the batch's result not collected
    sc.batch_result()
    recs, rec_off = sc.verify_batch_device()            # verify, then match, on one scan
    got = sc.match_batch_device()
    same(got, want)
    assert len(recs) >= len(got[0]) + len(got[2]) and rec_off[-1] == len(recs)
    again = sc.match_batch_device()                     # twice on one scan
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    # a single-block call between batches is unaffected, and leaves them so
    tm.assert_fields(sc.string_matches(data)[0], block_want, MATCH_FIELDS)
    _refused(sc.match_batch_device)
    same(sc.batch_string_matches(pieces), want)
    tm.assert_fields(sc.string_matches(data)[0], block_want, MATCH_FIELDS)
    # yr_amd_match_device keeps refusing a batch
    sc.batch_candidates(pieces)
    _refused(sc.match_device)
    # tables without strings
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(tables_npz("lit"), device=0))
    bare.batch_candidates(pieces)
    _refused(bare.match_batch_device)
    _refused(lambda: bare.batch_string_matches(pieces))
    # profiling tables (their own: the setting is the tables')
    tp = yara_amd.Tables.from_npz(tables_npz("lit"), device=0, strings=True)
    tp.set_profiling(True)
    sp = yara_amd.Scanner(tp)
    sp.scan_batch_device(d.data_ptr(), data.size, starts, sizes)
    sp.batch_result()
    _refused(sp.match_batch_device)
    _refused(lambda: sp.batch_string_matches(pieces))
    tp.set_profiling(False)
    same(sp.match_batch_device(), want)                 # the same scan, now served
    same(sp.batch_string_matches(pieces), want)
    torch.cuda.synchronize()
