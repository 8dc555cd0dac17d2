"""GPU: the hex class of the BATCH match stage
(yr_amd_scanner_set_batch_match_classes).  Buffer k of a batch must get exactly
what the single-block call with the hex class gives for that buffer alone
(Scanner.string_matches(hex=True), which test_gpu_hex_matches.py pins to stock
libyara); here the batch is pinned to that call, to the restatement of
test_gpu_hex_matches.py over each buffer's own records, and to stock libyara's
lists.  The CSR over items is walked through its edges: records, items and
matches that all differ per buffer, the sort's buffer passes, buffers cut
inside a match.  Every comparison is exact equality."""
import numpy as np
import pytest

import yara_amd
from yara_amd import _lib
from conftest import case_arrays, case_data, golden, tables_npz
from test_gpu_parity import blocks
from test_hex_match_abi import class_rule
from test_gpu_hex_matches import (EDGE_ITEMS, FOUR, ONE, SAME_START, SHORTEST, TWICE, TWO_BACK, WIDE,
                                  BLOCKS, WHOLE, assert_fields, assert_restated, cpu_records,
                                  edge_buffer, fixture, golden_matches, npz, restate, str_tables)
from test_gpu_batch_matches import MATCH_FIELDS, REST_FIELDS, same, singles

pytestmark = pytest.mark.gpu

LIT, HEX = yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX
INV = yara_amd.INVALID_ARGUMENT
CASES = golden()["cases"]
_RESTATED = {}


def hex_scanner(rules):
    """A scanner whose SINGLE-block calls settle hex strings too: what
    `singles` then returns is what a hex batch must give."""
    sc = yara_amd.Scanner(str_tables(rules))
    sc.set_match_classes(LIT | HEX)
    return sc


def restated(rules, piece):
    """restate() of a buffer's own records, computed once per distinct content."""
    key = (rules, piece.tobytes())
    if key not in _RESTATED:
        _RESTATED[key] = restate(rules, piece, cpu_records(rules, piece))
    return _RESTATED[key]


def assert_restated_batch(got, rules, pieces):
    m, mo, r, ro = got
    assert len(mo) == len(ro) == len(pieces) + 1 and mo[0] == 0 and ro[0] == 0
    assert mo[-1] == len(m) and ro[-1] == len(r)
    for k, p in enumerate(pieces):
        want, want_rest, _ = restated(rules, p)
        assert_restated(m[int(mo[k]):int(mo[k + 1])], want)
        # (the restatement's records carry no candidate index)
        assert_fields(r[int(ro[k]):int(ro[k + 1])], want_rest, ("offset", "pool_index"))


def class_strings_in(rules, rest):
    z = npz(rules)
    s = z["pool_string"][rest["pool_index"]]
    return set(s[class_rule(z["str_flags"], LIT | HEX)[s]].tolist())


def plant(size, *units):
    buf = np.zeros(size, np.uint8)
    for at, b in units:
        b = np.frombuffer(b, np.uint8)[:max(0, size - at)]
        buf[at:at + len(b)] = b
    return buf


# -- 1. per-buffer parity with the single-block hex call ------------------------------
GAP = np.frombuffer(FOUR + bytes.fromhex("d5d6d5d6") + bytes.fromhex("e1") + ONE[:4], np.uint8)


def gap_arena(pieces):
    """Gaps of 16..47 bytes before every buffer and behind the last, filled with
    bytes of the fixture's patterns: a run that left its buffer would go on."""
    starts, at = [], 32
    for p in pieces:
        starts.append(at)
        at = (at + len(p) + 15) // 16 * 16 + 32
    arena = np.resize(GAP, at).copy()
    for a, p in zip(starts, pieces):
        arena[a:a + len(p)] = p
    return arena, np.array(starts, np.uint64), np.array([len(p) for p in pieces], np.uint64)


def parity_pieces(name):
    if name == "hexmatch":
        data = fixture()[1]["data"]
        # inside the 4-offset $two_back copy (256..268), inside a $shortest copy
        # (512..521), between $same_start's two records (769, 773), an empty one
        edges = [0, 5, 258, 262, 300, 516, 516, 770, 1100, 1560, 2104, 3100, 4200, 20000, data.size]
        return "hexmatch", data, edges
    data = case_data(CASES["hex_1M"])
    rng = np.random.default_rng(12)
    e = sorted(int(x) for x in rng.integers(1, data.size, 10))
    return "hex", data, [0] + e[:5] + [e[4]] + e[5:] + [data.size]


@pytest.mark.parametrize("name", ["hexmatch", "hex_1M"])
def test_per_buffer_parity(name):
    import torch
    rules, data, edges = parity_pieces(name)
    pieces = [data[a:b] for a, b in zip(edges[:-1], edges[1:])]
    assert 12 <= len(pieces) <= 14 and min(len(p) for p in pieces) == 0
    assert len(set(len(p) for p in pieces)) >= len(pieces) - 1
    sc = hex_scanner(rules)
    arena, starts, sizes = gap_arena(pieces)
    dev = torch.from_numpy(arena).cuda()
    assert dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    lit = yara_amd.Scanner(str_tables(rules)).batch_string_matches(pieces)
    for bases in (None, np.array([k * 0x1000 + 7 for k in range(len(pieces))], np.uint64)):
        want = singles(sc, pieces, bases)
        got = sc.batch_string_matches(pieces, bases, hex=True)
        same(got, want)
        sc.scan_batch_device(dev.data_ptr(), len(arena), starts, sizes)
        sc.batch_result()
        same(sc.match_batch_device(bases, hex=True), want)
        # the feature is there: more matches and a shorter rest than literal-only
        assert len(got[0]) > len(lit[0]) + 10 and len(got[2]) < len(lit[2])
        # no record of the classes' strings is left but $wide's (hex_1M: none)
        assert class_strings_in(rules, got[2]) == ({WIDE} if name == "hexmatch" else set())
    torch.cuda.synchronize()


# -- 2. buffer edges: every cut through a backward and a forward run ------------------
def test_buffer_edges():
    data = plant(64, (8, FOUR), (40, ONE))
    sc = hex_scanner("hexmatch")
    whole = sc.string_matches(data)[0]
    assert list(whole["offset"][whole["string"] == TWO_BACK]) == [8, 9, 10, 11]
    assert list(whole["offset"][whole["string"] == SHORTEST]) == [40]
    cut_back, cut_fwd, adjacent = 0, 0, 0
    for c in range(data.size + 1):
        pieces = [data[:c], data[c:]]
        got = sc.batch_string_matches(pieces, hex=True)
        same(got, singles(sc, pieces))
        assert_restated_batch(got, "hexmatch", pieces)
        m, mo = got[0], got[1]
        for k, p in enumerate(pieces):
            mk = m[int(mo[k]):int(mo[k + 1])]
            # no match starts before the buffer's byte 0 or ends past its last byte
            assert np.all(mk["offset"] + mk["length"] <= len(p))
        first, second = m[:int(mo[1])], m[int(mo[1]):]
        if 9 <= c <= 11:
            # the backward run cut at the second buffer's byte 0: only the starts inside
            assert list(second["offset"][second["string"] == TWO_BACK]) == list(range(0, 12 - c))
            assert not (first["string"] == TWO_BACK).any()
            cut_back += 1
        if 12 <= c < 8 + len(FOUR) or 41 <= c < 40 + len(ONE):
            # the forward run's continuation lies in the next buffer: no match
            string = TWO_BACK if c < 32 else SHORTEST
            assert not (m["string"] == string).any()
            cut_fwd += 1
        adjacent += c % 16 == 0 and 0 < c < data.size
    assert (cut_back, cut_fwd, adjacent) == (3, 9 + 5, 3)


# -- 3. the items' CSR: records, items and matches that all differ per buffer ---------
@pytest.mark.parametrize("reverse", [False, True])
def test_items_csr_edges(reverse):
    order = EDGE_ITEMS[::-1] if reverse else EDGE_ITEMS
    pieces = [edge_buffer(items) for items in order]
    for items, p in zip(order, pieces):
        want, want_rest, n_items = restated("hexmatch", p)
        assert n_items == items and len(want_rest) == 0
    sc = yara_amd.Scanner(str_tables("hexmatch"))
    got = sc.batch_string_matches(pieces, hex=True)
    assert_restated_batch(got, "hexmatch", pieces)
    assert len(got[2]) == 0
    assert list(np.diff(got[1].astype(np.int64))) == [i - 100 if i >= 1000 else i for i in order]


def test_items_csr_interleaved():
    data = fixture()[1]["data"]
    wide = data[1016:1400]              # $wide's three records, nothing else
    e = np.zeros(0, np.uint8)
    pieces = []
    for items in EDGE_ITEMS:
        pieces += [edge_buffer(items), e, wide] if items % 2 else [e, e, edge_buffer(items)]
    pieces += [wide, e]
    want, want_rest, n_items = restated("hexmatch", wide)
    assert n_items == 0 and len(want_rest) == 3
    sc = hex_scanner("hexmatch")
    got = sc.batch_string_matches(pieces, hex=True)
    assert_restated_batch(got, "hexmatch", pieces)
    m, mo, r, ro = got
    assert class_strings_in("hexmatch", r) == {WIDE}
    assert set(npz("hexmatch")["pool_string"][r["pool_index"]].tolist()) == {WIDE}
    # record, item and match slot ranges all differ
    recs, rec_off = sc.batch_verify_calls(pieces)
    n_rec = np.diff(rec_off.astype(np.int64))
    n_items = np.array([restated("hexmatch", p)[2] for p in pieces])
    n_match = np.diff(mo.astype(np.int64))
    assert (n_rec != n_items).any() and (n_items != n_match).any() and (n_rec != n_match).any()
    assert list(np.diff(ro.astype(np.int64))) == [3 if p is wide else 0 for p in pieces]
    same(got, singles(sc, pieces))


# -- 4. distinct matches per buffer, the first record wins ------------------------------
def test_distinct_per_buffer_first_record_wins():
    p = plant(70, (3, TWICE), (35, TWICE))
    q = plant(41, (7, ONE))
    recs = cpu_records("hexmatch", p)
    z = npz("hexmatch")
    mine = recs[z["pool_string"][recs["pool_index"]] == SAME_START]
    assert len(mine) == 4                           # two records per copy, one offset each
    sc = hex_scanner("hexmatch")
    mp, mq = sc.string_matches(p)[0], sc.string_matches(q)[0]
    assert len(mp) == 2 and len(mq) == 1
    m, mo, r, ro = sc.batch_string_matches([p, p, q, p], hex=True)
    assert list(mo) == [0, 2, 4, 5, 7] and len(r) == 0
    for k, want in enumerate((mp, mp, mq, mp)):
        assert_fields(m[int(mo[k]):int(mo[k + 1])], want, MATCH_FIELDS)
    for k in (0, 1, 3):
        mk = m[int(mo[k]):int(mo[k + 1])]
        assert list(mk["string"]) == [SAME_START] * 2 and list(mk["offset"]) == [3, 35]
        assert list(mk["length"]) == [5, 5]
        assert list(mk["pool_index"]) == [int(mine[0]["pool_index"]), int(mine[2]["pool_index"])]


# -- 5. stock libyara --------------------------------------------------------------------
@pytest.mark.parametrize("case", BLOCKS)
def test_overlapping_blocks_in_one_batch(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = yara_amd.Scanner(str_tables(rec["rules"]))
    cut = list(blocks(data.size, rec["block"], rec["overlap"]))
    assert len(cut) > 1
    bases = np.array([b for b, _ in cut], np.uint64)
    m, mo, _, _ = sc.batch_string_matches([data[b:b + n] for b, n in cut], bases, hex=True)
    per = [(int(b), m[int(mo[k]):int(mo[k + 1])]) for k, (b, _) in enumerate(cut)]
    assert_fields(yara_amd.merge_matches(per), golden_matches(case_arrays(case), rec["rules"]))


@pytest.mark.parametrize("case", WHOLE)
def test_whole_goldens(case):
    rec = CASES[case]
    data = case_data(rec)
    sc = hex_scanner(rec["rules"])
    batch = [data[:0], data, data[:1000]]
    if case == "root_4K":   # root-accepting rules: such buffers are scanned one by one
        with pytest.raises(yara_amd.YaraAmdError) as e:
            sc.batch_string_matches(batch, hex=True)
        assert e.value.code == INV
        return
    m, mo, r, ro = sc.batch_string_matches(batch, hex=True)
    assert mo[0] == mo[1] == 0 and ro[0] == ro[1] == 0
    assert_fields(m[int(mo[1]):int(mo[2])], golden_matches(case_arrays(case), rec["rules"]))
    wm, wr = sc.string_matches(batch[2])
    assert_fields(m[int(mo[2]):], wm, MATCH_FIELDS)
    assert_fields(r[int(ro[2]):], wr, REST_FIELDS)


# -- 6. many buffers: the sort's buffer passes over items ---------------------------------
def test_4096_small_buffers():
    """12 buffer bits: one full pass and one partial."""
    rng = np.random.default_rng(7)
    n = 4096
    sizes = rng.integers(32, 97, n)
    for a in (0, 700, 701, n - 3):   # runs of empty buffers, at both ends too
        sizes[a:a + 3] = 0
    sizes[1000:1100] = 0
    units = (FOUR, ONE, TWICE, None)
    pieces = []
    for s in sizes:
        u = units[int(rng.integers(0, 4))]
        # (a unit may straddle the buffer's end: cut there)
        pieces.append(plant(int(s), (int(rng.integers(0, max(int(s), 1))), u)) if u is not None and s
                      else np.zeros(int(s), np.uint8))
    sc = hex_scanner("hexmatch")
    got = sc.batch_string_matches(pieces, hex=True)
    assert len(got[0]) > 2500 and len(got[2]) == 0
    same(got, singles(sc, pieces))


def test_65537_buffers():
    """17 buffer bits: three buffer passes."""
    kinds = [plant(32, (3, FOUR)), plant(32, (10, ONE)), plant(32, (3, TWICE)), np.zeros(32, np.uint8),
             plant(32, (22, FOUR)), plant(32, (0, FOUR[2:])), plant(32, (1, ONE), (12, TWICE))]
    rng = np.random.default_rng(8)
    n = 65537
    pick = rng.integers(0, len(kinds), n)
    pieces = [kinds[k] for k in pick]
    want = [restated("hexmatch", p) for p in kinds]
    assert sorted(len(w[0]["string"]) for w in want) == [0, 0, 1, 1, 2, 2, 4]
    sc = hex_scanner("hexmatch")
    m, mo, r, ro = sc.batch_string_matches(pieces, hex=True)
    assert len(r) == 0 and not ro.any()
    counts = np.array([len(w[0]["string"]) for w in want], np.int64)
    np.testing.assert_array_equal(mo, np.concatenate([[0], np.cumsum(counts[pick])]).astype(np.uint64))
    for f in ("string", "offset", "length", "pool_index"):   # (hex only: every length is restated)
        col = [w[0][f] for w in want]
        np.testing.assert_array_equal(m[f], np.concatenate([col[k] for k in pick]), err_msg=f)
    assert not m["xor_key"].any()
    sample = sorted(set(rng.integers(0, n, 62).tolist()) | {0, n - 1})
    for k in sample:
        wm, wr = sc.string_matches(pieces[k])
        np.testing.assert_array_equal(m[int(mo[k]):int(mo[k + 1])], wm, err_msg=str(k))
        assert len(wr) == 0


# -- 7. degenerate batches ---------------------------------------------------------------
def test_one_buffer_and_empty_batches():
    data = fixture()[1]["data"]
    sc = hex_scanner("hexmatch")
    got = sc.batch_string_matches([data], hex=True)   # n == 1: no buffer pass
    assert len(got[0]) > 15
    same(got, singles(sc, [data]))
    e = np.zeros(0, np.uint8)
    for pieces in ([], [e, e, e]):
        m, mo, r, ro = sc.batch_string_matches(pieces, hex=True)
        assert len(m) == 0 and len(r) == 0
        assert np.array_equal(mo, np.zeros(len(pieces) + 1)) and mo.dtype == np.uint64
        assert np.array_equal(ro, np.zeros(len(pieces) + 1)) and ro.dtype == np.uint64
        assert m.dtype == np.dtype(_lib.MATCH_REC_DTYPE) and r.dtype == np.dtype(_lib.VERIFY_REC_DTYPE)
    m, mo, r, ro = sc.batch_string_matches_device([], hex=True)
    assert len(m) == 0 and len(r) == 0 and list(mo) == [0] and list(ro) == [0]


# -- 8. buffers scattered in device memory -------------------------------------------------
def test_gather_path():
    import torch
    from test_gpu_gather import _place
    _, data, edges = parity_pieces("hexmatch")
    pieces = [data[a:b] for a, b in zip(edges[:-1], edges[1:])]
    mis = [(7 * k + 1) % 16 | 1 for k in range(len(pieces))]   # odd byte offsets
    src, views, host = _place(pieces, mis)
    sc = yara_amd.Scanner(str_tables("hexmatch"))
    bases = np.array([k * 0x1000 + 7 for k in range(len(pieces))], np.uint64)
    for b in (None, bases):
        want = sc.batch_string_matches(pieces, b, hex=True)
        assert len(want[0]) > 10
        same(sc.batch_string_matches_device(views, b, hex=True), want)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), host)


# -- 9. the two settings are independent ------------------------------------------------------
def equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_settings_are_independent():
    _, data, edges = parity_pieces("hexmatch")
    pieces = [data[a:b] for a, b in zip(edges[:-1], edges[1:])]
    t = str_tables("hexmatch")
    fresh = yara_amd.Scanner(t).batch_string_matches(pieces)
    fresh_single = yara_amd.Scanner(t).string_matches(data)
    sc = yara_amd.Scanner(t)
    sc.set_batch_match_classes(LIT | HEX)
    with_hex = sc.batch_string_matches(pieces)
    assert len(with_hex[0]) > len(fresh[0])
    equal(sc.string_matches(data), fresh_single)     # the single-block call does not read it
    sc.set_batch_match_classes(LIT)
    equal(sc.batch_string_matches(pieces), fresh)
    # hex=True is the batch classes for one call
    equal(sc.batch_string_matches(pieces, hex=True), with_hex)
    equal(sc.batch_string_matches(pieces), fresh)
    # the single-block setting alone: batches stay what they were
    sc.set_match_classes(LIT | HEX)
    equal(sc.batch_string_matches(pieces), fresh)
    equal(sc.batch_string_matches(pieces, hex=True), with_hex)
    equal(sc.string_matches(data), yara_amd.Scanner(t).string_matches(data, hex=True))


# -- 10. one scanner, alternating: the shared workspace ------------------------------------------
def test_one_scanner_alternating():
    t = str_tables("hexmatch")
    data = fixture()[1]["data"]
    big = [edge_buffer(items) for items in (20000, 257, 0, 64)]
    small = [data[:5000], data[5000:5003]]
    block = edge_buffer(256)
    want_big = yara_amd.Scanner(t).batch_string_matches(big, hex=True)
    want_small = yara_amd.Scanner(t).batch_string_matches(small)
    want_block = yara_amd.Scanner(t).string_matches(block, hex=True)
    assert len(want_big[0]) > 20000 and len(want_small[0]) > 0 and len(want_block[0]) == 256
    sc = yara_amd.Scanner(t)
    equal(sc.batch_string_matches(big, hex=True), want_big)
    equal(sc.batch_string_matches(small), want_small)
    equal(sc.string_matches(block, hex=True), want_block)
    equal(sc.batch_string_matches(big, hex=True), want_big)
    # and the other way round, from a small workspace upwards
    sc = yara_amd.Scanner(t)
    equal(sc.string_matches(block, hex=True), want_block)
    equal(sc.batch_string_matches(small, hex=True), yara_amd.Scanner(t).batch_string_matches(small, hex=True))
    equal(sc.batch_string_matches(big), yara_amd.Scanner(t).batch_string_matches(big))
    equal(sc.batch_string_matches(big, hex=True), want_big)


# -- 11. misuse -------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(yara_amd.YaraAmdError) as e:
        call()
    assert e.value.code == INV


def test_misuse():
    import torch
    data = case_data(CASES["hex_1M"])[:1 << 18]
    pieces = [data[:70000], data[70000:150001]]
    sc = yara_amd.Scanner(str_tables("hex"))
    for classes in (0, HEX, 4, LIT | 4):
        _refused(lambda: sc.set_batch_match_classes(classes))
    want = sc.batch_string_matches(pieces, hex=True)
    assert len(want[0]) > 5
    # tables without the strings' programs
    bare = yara_amd.Scanner(yara_amd.Tables.from_npz(tables_npz("hex"), device=0, strings=True,
                                                     regex=False))
    lit_only = bare.batch_string_matches(pieces)
    bare.set_batch_match_classes(LIT | HEX)
    _refused(lambda: bare.batch_string_matches(pieces))
    d = torch.from_numpy(data.copy()).cuda()
    torch.cuda.synchronize()
    starts, sizes = [0, 70000], [70000, 80001]
    bare.scan_batch_device(d.data_ptr(), data.size, starts, sizes)
    bare.batch_result()
    _refused(bare.match_batch_device)
    bare.set_batch_match_classes(LIT)
    equal(bare.match_batch_device(), lit_only)
    equal(bare.batch_string_matches(pieces), lit_only)
    # profiling tables (their own: the setting is the tables')
    tp = yara_amd.Tables.from_npz(tables_npz("hex"), device=0, strings=True)
    tp.set_profiling(True)
    sp = yara_amd.Scanner(tp)
    sp.scan_batch_device(d.data_ptr(), data.size, starts, sizes)
    sp.batch_result()
    _refused(lambda: sp.match_batch_device(hex=True))
    _refused(lambda: sp.batch_string_matches(pieces, hex=True))
    tp.set_profiling(False)
    equal(sp.match_batch_device(hex=True), want)
    # after a single-block scan: refused, and the scanner is still good
    single = sc.string_matches(data, hex=True)
    _refused(lambda: sc.match_batch_device(hex=True))
    equal(sc.string_matches(data, hex=True), single)
    equal(sc.batch_string_matches(pieces, hex=True), want)
    # a batch scan whose result was not collected
    sc.scan_batch_device(d.data_ptr(), data.size, starts, sizes)
    _refused(lambda: sc.match_batch_device(hex=True))
    sc.batch_result()
    equal(sc.match_batch_device(hex=True), want)
    torch.cuda.synchronize()
