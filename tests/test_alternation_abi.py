"""CPU: alternation strings (yr_amd_tables_alternation_strings, yr_amd_scanner_set_alternations)
-- the class against a restatement of its three conditions, and a plain transcription of
yr_re_exec (re.c:1693-2068) as an ordered fiber list that equals stock libyara's match lists
on tests/golden/alternation and on rx_1M.  The GPU tests use the transcription as reference."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, case_data, golden, tables_npz

FIX = os.path.join(GOLDEN, "alternation")
ASCII, EXCLUDED = 0x08, 0x400 | 0x40 | 0x2000 | 0x4000 | 0x10 | 0x04 | 0x80 | 0x80000 | 0x600000
DOT_ALL = 0x20000
SIZES = {0xA0: 1, 0xA2: 2, 0xAE: 2, 0xA4: 3, 0xAF: 3, 0xA5: 34, 0xA7: 1, 0xA8: 1, 0xA9: 1, 0xAA: 1,
         0xAB: 1, 0xAC: 1, 0xAD: 1, 0xB4: 5, 0xB5: 5, 0xC0: 4, 0xC1: 4, 0xC2: 3}


def i16(c, at):
    v = c[at] | c[at + 1] << 8
    return v - 65536 if v & 0x8000 else v


def u16(c, at):
    return c[at] | c[at + 1] << 8


def byte_test(c, ip, ch, dot_all):
    op = c[ip]
    if op in (0xA0, 0xB4, 0xB5):
        return dot_all or ch != 0x0A
    if op in (0xA2, 0xAE):
        return (ch == c[ip + 1]) != (op == 0xAE)
    if op in (0xA4, 0xAF):
        return ((ch & c[ip + 2]) == c[ip + 1]) != (op == 0xAF)
    if op == 0xA5:
        return bool(c[ip + 2 + ch // 8] >> ch % 8 & 1) != bool(c[ip + 1])
    word = chr(ch).isalnum() and ch < 128 or ch == 0x5F
    return {0xA7: word, 0xA8: not word, 0xA9: ch in b" \t\r\n\v\f", 0xAA: ch not in b" \t\r\n\v\f",
            0xAB: 48 <= ch <= 57, 0xAC: not 48 <= ch <= 57}[op]


def sync(c, fibers, at):
    """_yr_re_fiber_sync of fibers[at] (re.c:1441-1683): the list with its clones in place."""
    seen, i, last = set(), at, at + 1
    while i < last:
        ip, rc = fibers[i]
        op = c[ip]
        if op in (0xC0, 0xC1):
            if c[ip + 1] in seen:
                del fibers[i]
                last -= 1
                continue
            seen.add(c[ip + 1])
            nxt, tgt = (ip + 4, rc), (ip + i16(c, ip + 2), rc)
            fibers[i:i + 1] = [nxt, tgt] if op == 0xC0 else [tgt, nxt]
            last += 1
        elif op == 0xC2:
            fibers[i] = (ip + i16(c, ip + 1), rc)
        elif op in (0xB4, 0xB5):
            mn, mx, rc = u16(c, ip + 1), u16(c, ip + 3), max(rc, 0)
            if rc < mn:
                fibers[i] = (ip, rc + 1)
                i += 1
            elif rc < mx:
                leave = [(ip + 5, -1)]
                sync(c, leave, 0)
                pair = [(ip, rc + 1)] + leave if op == 0xB4 else leave + [(ip, rc + 1)]
                fibers[i:i + 1] = pair
                i += len(pair)
                last += len(pair) - 1
            else:
                fibers[i] = (ip + 5, -1)
        else:
            i += 1


def re_exec(code, data, offset, back, dot_all, exhaustive, window=False):
    """yr_re_exec: the last bytes_matched written (None: -1), or, exhaustive, all of them.
    window: whether, no fiber ever killed by a MATCH, one is alive at input byte 64."""
    c, exhaustive = code, exhaustive or window
    maxb = min(offset if back else len(data) - offset, 4096)
    fibers, out, b = [(0, -1)], [], 0
    sync(c, fibers, 0)
    while fibers:
        kept = []
        for f in fibers:                                  # _yr_re_fiber_exists: the later twin dies
            if f not in kept:
                kept.append(f)
        fibers, i = kept, 0
        if window and b == 64:
            return maxb > 64 and any(c[ip] != 0xAD for ip, _ in fibers)
        while i < len(fibers):
            ip, rc = fibers[i]
            if c[ip] == 0xAD:
                out.append(b)
                if exhaustive:
                    del fibers[i]
                else:
                    del fibers[i:]                        # ACTION_KILL_TAIL
                continue
            ch = int(data[offset - 1 - b] if back else data[offset + b]) if b < maxb else None
            if ch is None or not byte_test(c, ip, ch, dot_all):
                del fibers[i]
                continue
            before = len(fibers)
            fibers[i] = (ip if c[ip] in (0xB4, 0xB5) else ip + SIZES[c[ip]], rc)
            sync(c, fibers, i)
            i += 1 + len(fibers) - before
        b += 1
    if window:
        return False
    if exhaustive:
        return sorted(set(out))
    return out[-1] if out else None


# -- the class, restated --------------------------------------------------------------------
def program_facts(c):
    """(loop-free, fiber bound) of one program."""
    seen, work = set(), [0]
    while work:
        ip = work.pop()
        while ip not in seen:
            if not 0 <= ip < len(c) or c[ip] not in SIZES:
                return False, 0
            seen.add(ip)
            op = c[ip]
            if op == 0xAD:
                break
            if op in (0xC0, 0xC1, 0xC2):
                d = i16(c, ip + (1 if op == 0xC2 else 2))
                if d <= 0:
                    return False, 0
                if op == 0xC2:
                    ip += d
                    continue
                work.append(ip + d)
            ip += SIZES[op]
    ids = [c[ip + 1] for ip in seen if c[ip] in (0xC0, 0xC1)]
    if len(seen) > 64 or len(ids) != len(set(ids)):
        return False, 0
    arrive, bound = {}, 0
    for ip in sorted(seen, reverse=True):
        op, nxt = c[ip], ip + SIZES[c[ip]]
        if op == 0xC2:
            arrive[ip] = arrive[ip + i16(c, ip + 1)]
        elif op in (0xC0, 0xC1):
            arrive[ip] = arrive[nxt] + arrive[ip + i16(c, ip + 2)]
        elif op in (0xB4, 0xB5):
            arrive[ip] = 1 + arrive[nxt] if u16(c, ip + 1) == 0 else 1
            bound += (u16(c, ip + 3) + 1) * (1 + arrive[nxt])
        else:
            arrive[ip] = 1
            bound += 1 if op == 0xAD else arrive[nxt]
    return True, bound + arrive[0]


def programs(z, k):
    code = [int(x) for x in z["re_code"]]
    fwd = code[z["re_fwd_off"][k]:z["re_fwd_off"][k] + z["re_fwd_len"][k]] if z["re_kind"][k] else []
    bwd = code[z["re_bwd_off"][k]:z["re_bwd_off"][k] + z["re_bwd_len"][k]] if fwd else []
    return fwd, bwd


def class_rule(z):
    flags = z["str_flags"]
    out = [bool(f & ASCII) and not f & EXCLUDED for f in flags]
    entries = [0] * len(flags)
    for k, s in enumerate(z["pool_string"]):
        entries[s] += 1
        for prog in programs(z, k) if out[s] else ():
            ok, bound = program_facts(prog) if prog else (prog is programs(z, k)[1], 0)
            out[s] = out[s] and ok and bound < 1024
    return np.array([o and e > 0 for o, e in zip(out, entries)])


def fixture():
    with open(os.path.join(FIX, "manifest.json")) as f:
        return json.load(f), dict(np.load(os.path.join(FIX, "case.npz"))), \
            dict(np.load(os.path.join(FIX, "tables.npz")))


def settle(z, data, recs, alt, window=True):
    """({(string, offset): length} of the alternation strings, the records of theirs left in
    the rest) of a record stream: scan.c:778-885 over the transcription.  window: with the
    device's 64-position window -- a run that needs input byte 64, or a backward
    bytes_matched of 64, leaves its record."""
    items, rest = {}, []
    for r, (off, k) in enumerate(recs):
        s = int(z["pool_string"][k])
        if not alt[s]:
            continue
        fwd, bwd = programs(z, k)
        dot_all = bool(z["str_flags"][s] & DOT_ALL)
        F = re_exec(fwd, data, off, False, dot_all, False)
        Bs = re_exec(bwd, data, off, True, dot_all, True) if bwd else ([0] if F else [])
        leaves = window and (re_exec(fwd, data, off, False, dot_all, True, True) or bool(bwd) and (
            re_exec(bwd, data, off, True, dot_all, True, True) or max(Bs, default=0) > 63))
        if F is None or not Bs or leaves:
            rest.append(r)
            continue
        for B in Bs:
            items.setdefault((s, off - B), B + F)
    return items, rest


def calls(a, z):
    """Stock's verify calls as (offset, pool index): the automaton's position less the backtrack."""
    return [(int(p) - int(z["pool_backtrack"][k]), int(k)) for p, k in
            zip(a["verify_pos"], a["verify_idx"])]


def stock_of(a, sel):
    keep = sel[a["match_string"]]
    return {(int(s), int(o)): int(n) for s, o, n in
            zip(a["match_string"][keep], a["match_offset"][keep], a["match_len"][keep])}


# -- tests ----------------------------------------------------------------------------------
def test_symbols():
    L = _lib.lib()
    assert L.yr_amd_scanner_set_alternations(None, 1) == yara_amd.INVALID_ARGUMENT
    out = (ctypes.c_uint8 * 4)()
    assert L.yr_amd_tables_alternation_strings(None, out, 4) == yara_amd.INVALID_ARGUMENT
    t = yara_amd.Tables.from_npz(tables_npz("rx"), device=-1)          # no flags, no programs
    assert L.yr_amd_tables_alternation_strings(t.handle, out, 4) == yara_amd.INVALID_ARGUMENT
    t = yara_amd.Tables.from_npz(tables_npz("rx"), device=-1, strings=True, regex=False)
    n = t.string_count()
    out = (ctypes.c_uint8 * n)()
    assert L.yr_amd_tables_alternation_strings(t.handle, out, n) == yara_amd.INVALID_ARGUMENT
    t = yara_amd.Tables.from_npz(tables_npz("rx"), device=-1, strings=True)
    assert L.yr_amd_tables_alternation_strings(t.handle, out, n) == yara_amd.SUCCESS
    assert L.yr_amd_tables_alternation_strings(t.handle, out, n + 1) == yara_amd.INVALID_ARGUMENT
    assert L.yr_amd_tables_alternation_strings(t.handle, None, n) == yara_amd.INVALID_ARGUMENT


@pytest.mark.parametrize("name", ["alternation", "rx", "hex", "lit"])
def test_class(name):
    path = os.path.join(FIX, "tables.npz") if name == "alternation" else tables_npz(name)
    z = dict(np.load(path))
    got = yara_amd.Tables.from_npz(path, device=-1, strings=True).alternation_strings()
    np.testing.assert_array_equal(got, class_rule(z))
    if name == "alternation":
        names = fixture()[0]["strings"]
        out = {"insns65", "far", "plus", "boundary", "nocase", "wide"}
        assert {names[k] for k in np.flatnonzero(~got)} == out
        with gzip.open(os.path.join(FIX, "rules.yarc.gz")) as f:
            yarc = yara_amd.Tables.from_yarc(f.read(), device=-1)
        np.testing.assert_array_equal(yarc.alternation_strings(), got)
    if name == "rx":
        assert got.sum() == 5                                          # $f, $g and the hex three


def one_string_tables(flags, code):
    """Host-only tables (lit's automaton) whose string 0 has these flags and, on each of its
    pool entries, this forward program; the other strings are literals."""
    z = np.load(tables_npz("lit"))
    t = yara_amd.Tables(z["T"], z["M"], z["pool_next"], z["pool_backtrack"], device=-1)
    fl = np.full(len(z["str_flags"]), 0x400 | ASCII, np.uint32)
    fl[0] = flags
    t.set_string_flags(fl)
    mine = (z["pool_string"] == 0).astype(np.uint32)
    assert mine.any()
    t._set_host_programs(z["pool_string"], 0 * mine, len(code) * mine, 0 * mine, 0 * mine,
                         np.array(code, np.uint8))
    return t


LIT4 = [0xA2, 1, 0xA2, 2, 0xA2, 3, 0xA2, 4]
BASE = LIT4 + [0xC0, 0, 9, 0, 0xA2, 5, 0xC2, 5, 0, 0xA2, 6, 0xAD]     # 01 02 03 04 ( 05 | 06 )


@pytest.mark.parametrize("flag", [0x400, 0x40, 0x2000, 0x4000, 0x10, 0x04, 0x80, 0x80000, 0x200000,
                                  0x400000])
def test_excluded_flags(flag):
    assert one_string_tables(0x2020A, BASE).alternation_strings()[0]
    assert one_string_tables(0x20202, BASE).alternation_strings()[0] == False   # noqa: E712 (no ASCII)
    assert not one_string_tables(0x2020A | flag, BASE).alternation_strings()[0]
    assert one_string_tables(0x2020A | 0x10000, BASE).alternation_strings()[0]   # GREEDY_REGEXP


def program_ok(code, bound):
    fn = _lib.lib().yr_amd__alternation_program           # (not part of the declared ABI)
    fn.restype, fn.argtypes = ctypes.c_int, [_lib._u8p, ctypes.c_uint32, ctypes.c_void_p]
    return fn(np.array(code, np.uint8).ctypes.data_as(_lib._u8p), len(code), bound)


REPEAT = [1, 0, 2, 0, 12, 0, 0, 0]                                     # {1, 2}, offset
@pytest.mark.parametrize("code", [
    LIT4 + [0xB2, 0xAD], LIT4 + [0xB3, 0xAD], LIT4 + [0xB0, 0xAD], LIT4 + [0xB1, 0xAD],
    LIT4 + [0xC3] + REPEAT + [0xA0, 0xC4] + REPEAT + [0xAD],
    LIT4 + [0xC5] + REPEAT + [0xA0, 0xC6] + REPEAT + [0xAD],
    [0xA2, 1, 0xC1, 0, 0xFE, 0xFF, 0xAD],                              # a+: a backward SPLIT
    [0xC0, 0, 9, 0, 0xA2, 1, 0xC2, 0xFA, 0xFF, 0xAD],                  # a*: a backward JUMP
    LIT4 + [0xC0, 0, 6, 0, 0xA2, 5, 0xC0, 0, 4, 0, 0xA2, 6, 0xAD],     # one split id twice
])
def test_excluded_opcodes(code):
    assert not one_string_tables(0x2020A, code).alternation_strings()[0]
    assert program_ok(code, None) == 0


def test_fiber_bound_edge():
    def bound_of(code):
        b = ctypes.c_uint64()
        ok = program_ok(code, ctypes.byref(b))
        free, bound = program_facts(code)
        assert (ok == 1, b.value) == (free and bound < 1024, bound)
        return ok, b.value
    # LITERAL, REPEAT_ANY {0, mx}, LITERAL, MATCH: 2 + (mx + 1) * 2 + 1 + 1 + the entry's 1
    at = lambda mx: [0xA2, 1, 0xB5, 0, 0, mx & 0xFF, mx >> 8, 0xA2, 2, 0xAD]   # noqa: E731
    assert bound_of(at(508)) == (1, 1023) and bound_of(at(509)) == (0, 1025)
    assert one_string_tables(0x2020A, at(508)).alternation_strings()[0]
    assert not one_string_tables(0x2020A, at(509)).alternation_strings()[0]
    insns = lambda n: LIT4[:2] * (n - 1) + [0xAD]                      # noqa: E731
    assert bound_of(insns(64))[0] == 1 and bound_of(insns(65))[0] == 0


def test_transcription_equals_stock_on_the_fixture():
    man, a, z = fixture()
    alt, recs = class_rule(z), calls(a, z)
    want, names = stock_of(a, alt), man["strings"]
    assert settle(z, a["data"], recs, alt, window=False)[0] == want
    items, rest = settle(z, a["data"], recs, alt)
    lost = (names.index("run65"), 896)                                 # the window's one loss
    assert {**items, lost: 65} == want and lost not in items
    assert sum((int(z["pool_string"][recs[r][1]]), recs[r][0]) == lost for r in rest) == 1
    s = names.index                                                    # the shapes it is there for
    assert want[s("long_first"), 128] == 9 and want[s("short_first"), 192] == 7
    assert want[s("before"), 256] == 8 and want[s("before"), 257] == 7 and want[s("before"), 0] == 7
    assert want[s("run63"), 640] == 63 and want[s("run64"), 768] == 64
    assert want[s("greedy"), 1344] == 7 and want[s("ungreedy"), 1352] == 5
    assert (s("greedy"), 1408) not in want and want[s("greedy_s"), 1420] == 5
    assert want[s("animals"), man["size"] - 9] == 9


def test_transcription_equals_stock_on_both():
    """Chains beside alternation strings (both.yar).  `edge`, its atom at offset 64: backwards the
    long alternative is alive at position 64, where max_bytes_matched ends it, and the short one
    has matched 63 bytes -- inside the window, so the record is settled."""
    z, a = dict(np.load(os.path.join(FIX, "both_tables.npz"))), dict(np.load(os.path.join(FIX, "both_case.npz")))
    alt = class_rule(z)
    got = yara_amd.Tables.from_npz(os.path.join(FIX, "both_tables.npz"), device=-1, strings=True)
    np.testing.assert_array_equal(got.alternation_strings(), alt)
    assert list(np.flatnonzero(alt)) == [2, 3, 8]                      # long_first, before, edge
    items, rest = settle(z, a["data"], calls(a, z), alt)
    assert items == stock_of(a, alt) and not rest and items[8, 1] == 67 and len(items) == 8


def test_transcription_equals_stock_on_rx_1M():
    z, a = dict(np.load(tables_npz("rx"))), dict(np.load(os.path.join(GOLDEN, "cases", "rx_1M.npz")))
    alt = class_rule(z)
    recs = [r for r in calls(a, z) if alt[z["pool_string"][r[1]]]]
    data = case_data(golden()["cases"]["rx_1M"])
    assert recs and settle(z, data, recs, alt, window=False)[0] == stock_of(a, alt)
