"""CPU: loop strings (yr_amd_tables_loop_strings, yr_amd_scanner_set_loops) -- the class on
tests/golden/loops against its manifest, the arguments, and the edges of the class on one program."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, tables_npz

FIX = os.path.join(GOLDEN, "loops")


def fixture():
    with open(os.path.join(FIX, "manifest.json")) as f:
        return json.load(f), dict(np.load(os.path.join(FIX, "case.npz"))), \
            dict(np.load(os.path.join(FIX, "tables.npz")))


def test_class_is_the_manifests():
    man = fixture()[0]
    t = yara_amd.Tables.from_npz(os.path.join(FIX, "tables.npz"), device=-1, strings=True)
    names = np.array(man["strings"])
    assert list(names[t.loop_strings()]) == man["loop_strings"]
    assert list(names[t.alternation_strings()]) == man["alternation_strings"]
    assert not (t.loop_strings() & t.alternation_strings()).any()
    with gzip.open(os.path.join(FIX, "rules.yarc.gz")) as f:
        yarc = yara_amd.Tables.from_yarc(f.read(), device=-1)
    np.testing.assert_array_equal(yarc.loop_strings(), t.loop_strings())
    rx = yara_amd.Tables.from_npz(tables_npz("rx"), device=-1, strings=True)
    assert list(np.flatnonzero(rx.loop_strings())) == [4]              # /GET \/[a-z]+\.php\?id=[0-9]+/
    assert not (rx.loop_strings() & rx.alternation_strings()).any()


def test_stock_lists_hold_the_shapes():
    man, a, _ = fixture()
    s = man["strings"].index
    got = {(int(k), int(o)): int(n) for k, o, n in zip(a["match_string"], a["match_offset"], a["match_len"])}
    assert got[s("plus"), 65] == 7 and got[s("star"), 83] == 4 and got[s("plus_u"), 89] == 5
    assert got[s("star_u"), 98] == 4 and got[s("alt"), 129] == 9 and got[s("php"), 0] == 6
    assert [got[s("run"), o] for o in (257, 385, 513)] == [63, 64, 65]
    assert [got[s("dot"), o] for o in (2048, 6400, 10752)] == [4095, 4096, 100]
    assert got[s("coll_g"), 641] == 9 and got[s("coll_u"), 705] == 5   # replace_if_exists
    assert (s("line"), 769) not in got and got[s("line_s"), 780] == 18
    assert got[s("plus"), man["size"] - 7] == 7 and got[s("php"), 1153] == 68


def test_arguments():
    L = _lib.lib()
    out = (ctypes.c_uint8 * 4)()
    assert L.yr_amd_scanner_set_loops(None, 1) == yara_amd.INVALID_ARGUMENT
    assert L.yr_amd_tables_loop_strings(None, out, 4) == yara_amd.INVALID_ARGUMENT
    t = yara_amd.Tables.from_npz(tables_npz("rx"), device=-1, strings=True, regex=False)
    n = t.string_count()
    out = (ctypes.c_uint8 * n)()
    assert L.yr_amd_tables_loop_strings(t.handle, out, n) == yara_amd.INVALID_ARGUMENT   # no programs
    t = yara_amd.Tables.from_npz(tables_npz("rx"), device=-1, strings=True)
    assert L.yr_amd_tables_loop_strings(t.handle, out, n) == yara_amd.SUCCESS
    assert L.yr_amd_tables_loop_strings(t.handle, out, n + 1) == yara_amd.INVALID_ARGUMENT
    assert L.yr_amd_tables_loop_strings(t.handle, None, n) == yara_amd.INVALID_ARGUMENT


def program(code):
    """(in the class, fiber bound, has a backward edge) of one program."""
    fn = _lib.lib().yr_amd__loop_program                               # (not part of the declared ABI)
    fn.restype, fn.argtypes = ctypes.c_int, [_lib._u8p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    bound, back = ctypes.c_uint64(), ctypes.c_int()
    ok = fn(np.array(code, np.uint8).ctypes.data_as(_lib._u8p), len(code), ctypes.byref(bound),
            ctypes.byref(back))
    return ok, bound.value, back.value


def optional(k):
    return [0xC0, k, 6, 0, 0xA2, 1]                                    # (a?): SPLIT_A id k over LITERAL


PLUS = lambda k: [0xA2, 1, 0xC1, k, 0xFE, 0xFF]                        # noqa: E731  a+: SPLIT_B back
EMPTY = lambda k: [0xC0, k, 4, 0]                                      # noqa: E731  both ways to next


def test_fiber_bound_edge():
    # resting x (splits + 1): 29 optional + a+ + two empty splits + MATCH = 31 x 33, one below
    # RE_MAX_FIBERS; 30 optional + a+ + MATCH = 32 x 32, RE_MAX_FIBERS itself
    inside = sum((optional(k) for k in range(29)), []) + PLUS(29) + EMPTY(30) + EMPTY(31) + [0xAD]
    outside = sum((optional(k) for k in range(30)), []) + PLUS(30) + [0xAD]
    assert program(inside) == (1, 1023, 1) and program(outside) == (0, 1024, 1)


@pytest.mark.parametrize("code,ok", [
    ([0xA2, 1] * 61 + PLUS(0) + [0xAD], 1),                            # 64 instructions
    ([0xA2, 1] * 62 + PLUS(0) + [0xAD], 0),                            # 65
    ([0xC0, 0, 16, 0, 0xC0, 1, 9, 0, 0xA2, 1, 0xC2, 0xFA, 0xFF, 0xC2, 0xF3, 0xFF, 0xA2, 2, 0xAD], 0),  # (a*)*b
    ([0xA2, 1, 0xB4, 1, 0, 3, 0, 0xA2, 2, 0xC1, 0, 0xFE, 0xFF, 0xAD], 0),   # REPEAT_ANY beside a loop
    (optional(0) + PLUS(0) + [0xAD], 0),                               # one split id twice
    (PLUS(0) + [0xB2, 0xAD], 0),                                       # \b
])
def test_class_edges(code, ok):
    assert program(code)[0] == ok
