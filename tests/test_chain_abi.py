"""Chained strings without a GPU: the new symbols, the settled-chain rule
(yr_amd_tables_chain_strings) on host-only tables, every refusal of yr_amd_tables_set_chains."""
import gzip
import os
import re

import numpy as np
import pytest

import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, REPO, tables_npz
from test_hex_match_abi import class_rule

NEW = ("yr_amd_tables_set_chains", "yr_amd_tables_chain_strings", "yr_amd_scanner_set_chains")
LIT, HEX = 1, 2
PART, TAIL, LITERAL, XOR = 0x2000, 0x4000, 0x400, 0x80000
NONE = 0xFFFFFFFF
CHAIN = os.path.join(GOLDEN, "chain", "tables.npz")


def chain_rule(flags, to, classes):
    """Part of a chain whose every string, the chain bits masked off, is in the classes and
    carries no XOR."""
    f = np.asarray(flags, np.uint32)
    ok = class_rule(f & ~np.uint32(PART | TAIL), classes) & ((f & XOR) == 0)
    out = np.zeros(len(flags), bool)
    for k in range(len(flags)):
        if to[k] != NONE and k not in set(to):   # a tail: up to its head
            parts = [k]
            while to[parts[-1]] != NONE:
                parts.append(to[parts[-1]])
            out[parts] = ok[parts].all()
    return out


def test_symbols():
    L = _lib.lib()
    with open(os.path.join(REPO, "include", "yara_amd.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES
        assert re.search(r"\bint %s\(" % name, header)
    assert re.search(r"int yr_amd_tables_set_chains\(\s*yr_amd_tables\* tables,\s*const uint32_t\* "
                     r"chained_to,\s*const int32_t\* gap_min,\s*const int32_t\* gap_max,\s*"
                     r"uint32_t n_strings\);", header)
    assert "int yr_amd_scanner_set_chains(yr_amd_scanner* scanner, int enable);" in header
    assert L.yr_amd_scanner_set_chains(None, 1) == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("classes", [LIT, LIT | HEX])
def test_chain_strings_equal_the_rule(classes):
    z = np.load(CHAIN)
    t = yara_amd.Tables.from_npz(CHAIN, device=-1, strings=True)
    got = t.chain_strings(classes)
    np.testing.assert_array_equal(got, chain_rule(z["str_flags"], z["str_chained_to"], classes))
    assert got.sum() == (7 if classes == LIT else 13)   # two, three, open; + wild, dirty, vary
    assert not got[[13, 14]].any() and (z["str_chained_to"][14], z["str_flags"][13] & PART) == (13, PART)   # the regexp's chain
    np.testing.assert_array_equal(t.match_strings(classes), class_rule(z["str_flags"], classes))
    with gzip.open(os.path.join(GOLDEN, "yarc", "hex.yarc.gz")) as f:
        y = yara_amd.Tables.from_yarc(f.read(), device=-1)
    assert list(np.nonzero(y.chain_strings(classes))[0]) == [9, 10]
    for bad in (0, HEX, 4, LIT | 4):
        with pytest.raises(yara_amd.YaraAmdError):
            t.chain_strings(bad)
    # tables without chain records
    bare = yara_amd.Tables.from_npz(tables_npz("hex"), device=-1, strings=True)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.chain_strings(classes)
    assert e.value.code == _lib.INVALID_ARGUMENT


def set_chains(flags, to, lo, hi):
    t = yara_amd.Tables.from_npz(tables_npz("hex"), device=-1)
    t.set_string_flags(np.asarray(flags, np.uint32))
    t.set_chains(to, lo, hi)
    return t


H, M, T = LITERAL | PART, LITERAL | PART, LITERAL | PART | TAIL
REFUSED = {
    "index out of range": ([H, T], [NONE, 2], [0, 1], [0, 2]),
    "chained to itself": ([H, T], [NONE, 1], [0, 1], [0, 2]),
    "cycle": ([M, M], [1, 0], [1, 1], [2, 2]),
    "negative gap": ([H, T], [NONE, 0], [0, -1], [0, 2]),
    "gap_max < gap_min": ([H, T], [NONE, 0], [0, 3], [0, 2]),
    "link without CHAIN_PART": ([H, LITERAL | TAIL], [NONE, 0], [0, 1], [0, 2]),
    "last part without CHAIN_TAIL": ([H, M], [NONE, 0], [0, 1], [0, 2]),
    "two strings chained to one": ([H, T, T], [NONE, 0, 0], [0, 1, 1], [0, 2, 2]),
    "link to a string without CHAIN_PART": ([LITERAL, T], [NONE, 0], [0, 1], [0, 2]),
    "CHAIN_TAIL on a middle part": ([H, T, T], [NONE, 0, 1], [0, 1, 1], [0, 2, 2]),
    "CHAIN_TAIL on a string without a link": ([H, T, LITERAL | TAIL], [NONE, 0, NONE], [0, 1, 0], [0, 2, 0]),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_set_chains_refuses(what):
    with pytest.raises(yara_amd.YaraAmdError) as e:
        set_chains(*REFUSED[what])
    assert e.value.code == _lib.INVALID_ARGUMENT


def test_set_chains_once():
    t = set_chains([H, T], [NONE, 0], [0, 1], [0, 2])
    with pytest.raises(yara_amd.YaraAmdError) as e:
        t.set_chains([NONE, 0], [0, 1], [0, 2])
    assert e.value.code == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("parts,settled", [(64, True), (65, False)])
def test_chain_length_limit(parts, settled):
    """A chain of more than 64 parts is valid and stays unsettled."""
    t = set_chains([H] + [M] * (parts - 2) + [T], [NONE] + list(range(parts - 1)), [0] + [1] * (parts - 1),
                   [0] + [2] * (parts - 1))
    assert list(t.chain_strings(LIT)) == [settled] * parts


def test_xor_part_is_not_settled():
    flags, to = [H, T | XOR, H, T], [NONE, 0, NONE, 2]
    t = set_chains(flags, to, [0, 1, 0, 1], [0, 2, 0, 2])
    assert list(t.chain_strings(LIT)) == [False, False, True, True]
    np.testing.assert_array_equal(t.chain_strings(LIT), chain_rule(flags, to, LIT))


def test_set_chains_arguments():
    t = set_chains([H, M, T, LITERAL], [NONE, 0, 1, NONE], [0, 1, 1, 0], [0, 2, 0x7FFFFFFF, 0])
    assert list(t.chain_strings(LIT)) == [True, True, True, False]
    L = _lib.lib()
    one = np.array([NONE], np.uint32).ctypes.data_as(_lib._u32p)
    gap = np.zeros(1, np.int32).ctypes.data_as(_lib._i32p)
    assert L.yr_amd_tables_set_chains(None, one, gap, gap, 1) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_tables_set_chains(t.handle, one, gap, gap, 1) == _lib.INVALID_ARGUMENT   # twice
    u = yara_amd.Tables.from_npz(tables_npz("hex"), device=-1)
    assert L.yr_amd_tables_set_chains(u.handle, one, gap, gap, 1) == _lib.INVALID_ARGUMENT   # no flags
    u.set_string_flags(np.array([LITERAL, LITERAL], np.uint32))
    assert L.yr_amd_tables_set_chains(u.handle, one, gap, gap, 1) == _lib.INVALID_ARGUMENT   # count
    assert L.yr_amd_tables_set_chains(u.handle, None, gap, gap, 2) == _lib.INVALID_ARGUMENT
    out = np.zeros(4, np.uint8).ctypes.data_as(_lib._u8p)
    assert L.yr_amd_tables_chain_strings(None, LIT, out, 4) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_tables_chain_strings(t.handle, LIT, out, 3) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_tables_chain_strings(t.handle, LIT, None, 4) == _lib.INVALID_ARGUMENT
