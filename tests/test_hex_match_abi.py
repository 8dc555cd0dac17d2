"""The hex class of the match stage without a GPU: the new symbols, the class
rule (yr_amd_tables_match_strings) on host-only tables, error behaviour."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, REPO, tables_npz
from test_match_abi import final_rule

TABLES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "tables", "*.npz")))
HEXMATCH = os.path.join(GOLDEN, "hexmatch", "tables.npz")
NEW = ("yr_amd_scanner_set_match_classes", "yr_amd_tables_match_strings")
LIT, HEX = 1, 2

FAST_REGEXP, ASCII = 0x40, 0x08
# LITERAL, CHAIN_PART, WIDE, NO_CASE, FULL_WORD, GREEDY_REGEXP, BASE64, BASE64_WIDE
EXCLUDED = 0x400 | 0x2000 | 0x10 | 0x04 | 0x80 | 0x10000 | 0x200000 | 0x400000


def hex_rule(flags):
    """The final hex strings of include/yara_amd.h, restated."""
    f = np.asarray(flags, np.uint32)
    return ((f & (FAST_REGEXP | ASCII)) == (FAST_REGEXP | ASCII)) & ((f & EXCLUDED) == 0)


def class_rule(flags, classes):
    out = np.zeros(len(flags), bool)
    if classes & LIT:
        out |= final_rule(flags)
    if classes & HEX:
        out |= hex_rule(flags)
    return out


def test_symbols():
    L = _lib.lib()
    with open(os.path.join(REPO, "include", "yara_amd.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
        assert re.search(r"\bint %s\(" % name, header)
    assert re.search(r"#define YR_AMD_MATCH_LITERAL 1u\b", header)
    assert re.search(r"#define YR_AMD_MATCH_HEX 2u\b", header)
    assert (yara_amd.MATCH_LITERAL, yara_amd.MATCH_HEX) == (LIT, HEX)
    assert {"MATCH_LITERAL", "MATCH_HEX"} <= set(yara_amd.__all__)


@pytest.mark.parametrize("name", TABLES + ["hexmatch"])
def test_match_strings_equal_the_class_rule(name):
    path = HEXMATCH if name == "hexmatch" else tables_npz(name)
    flags = np.load(path)["str_flags"]
    t = yara_amd.Tables.from_npz(path, device=-1, strings=True)
    lit = t.match_strings(LIT)
    both = t.match_strings(LIT | HEX)
    assert both.dtype == bool and both.shape == (len(flags),)
    np.testing.assert_array_equal(lit, t.final_strings())
    np.testing.assert_array_equal(t.match_strings(), lit)
    np.testing.assert_array_equal(lit, class_rule(flags, LIT))
    np.testing.assert_array_equal(both, class_rule(flags, LIT | HEX))
    assert not (hex_rule(flags) & final_rule(flags)).any()
    if name in ("hex", "C", "E", "hexmatch"):
        assert (both & ~lit).any()
    if name in ("short", "rx", "root"):
        np.testing.assert_array_equal(both, lit)


def test_hand_made_flags_fall_to_the_rest():
    """Each excluded flag alone takes a FAST_REGEXP | ASCII string out of the class."""
    bits = [0x400, 0x2000, 0x10, 0x04, 0x80, 0x10000, 0x200000, 0x400000]
    flags = np.array([FAST_REGEXP | ASCII] + [FAST_REGEXP | ASCII | b for b in bits] +
                     [FAST_REGEXP, ASCII, FAST_REGEXP | ASCII | 0x20000 | 0x8000], np.uint32)
    z = np.load(tables_npz("lit"))
    t = yara_amd.Tables(z["T"], z["M"], z["pool_next"], z["pool_backtrack"], device=-1)
    t.set_string_flags(flags)
    got = t.match_strings(LIT | HEX) & ~t.match_strings(LIT)
    want = np.zeros(len(flags), bool)
    want[0] = want[-1] = True
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, hex_rule(flags))


def test_invalid_arguments():
    L = _lib.lib()
    INV = yara_amd.INVALID_ARGUMENT
    z = np.load(tables_npz("hex"))
    n = len(z["str_flags"])
    out = np.zeros(n + 1, np.uint8)
    op = out.ctypes.data_as(_lib._u8p)
    assert L.yr_amd_tables_match_strings(None, LIT, op, n) == INV
    assert L.yr_amd_scanner_set_match_classes(None, LIT) == INV
    bare = yara_amd.Tables.from_npz(tables_npz("hex"), device=-1)
    assert L.yr_amd_tables_match_strings(bare.handle, LIT, op, n) == INV
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.match_strings(LIT | HEX)
    assert e.value.code == INV
    t = yara_amd.Tables.from_npz(tables_npz("hex"), device=-1, strings=True)
    for classes in (0, HEX, 4, LIT | 4, LIT | HEX | 8, 0x80000001):
        assert L.yr_amd_tables_match_strings(t.handle, classes, op, n) == INV, classes
    assert L.yr_amd_tables_match_strings(t.handle, LIT | HEX, op, n + 1) == INV
    assert L.yr_amd_tables_match_strings(t.handle, LIT | HEX, op, n - 1) == INV
    assert L.yr_amd_tables_match_strings(t.handle, LIT | HEX, None, n) == INV
    assert L.yr_amd_tables_match_strings(t.handle, LIT | HEX, op, n) == yara_amd.SUCCESS
    assert out[n] == 0
