"""The match stage's ABI without a GPU: record layout, the final-string rule
on host-only tables, merging the blocks of one scan, error behaviour."""
import ctypes
import glob
import os

import numpy as np
import pytest

import yara_amd
from yara_amd import _lib
from conftest import GOLDEN, tables_npz

LITERAL, CHAIN_PART, BASE64, BASE64_WIDE = 0x400, 0x2000, 0x200000, 0x400000
TABLES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "tables", "*.npz")))


def final_rule(flags):
    """The rule of include/yara_amd.h, restated: literal, not a chain part, not base64."""
    f = np.asarray(flags, np.uint32)
    return ((f & LITERAL) != 0) & ((f & (CHAIN_PART | BASE64 | BASE64_WIDE)) == 0)


def test_match_record_layout():
    assert ctypes.sizeof(_lib.MatchRec) == 24
    dt = np.dtype(_lib.MATCH_REC_DTYPE)
    assert dt.itemsize == 24
    want = {"offset": (0, 8), "string": (8, 4), "length": (12, 4), "xor_key": (16, 4),
            "pool_index": (20, 4)}
    assert set(dt.names) == set(want)
    for name, (off, size) in want.items():
        assert dt.fields[name][1] == off and dt.fields[name][0].itemsize == size
        assert getattr(_lib.MatchRec, name).offset == off and getattr(_lib.MatchRec, name).size == size


def test_tables_cover_every_golden_set():
    assert len(TABLES) >= 20 and {"hex", "rx", "lit", "short", "C"} <= set(TABLES)


@pytest.mark.parametrize("name", TABLES)
def test_final_strings_equal_the_flag_rule(name):
    flags = np.load(tables_npz(name))["str_flags"]
    t = yara_amd.Tables.from_npz(tables_npz(name), device=-1, strings=True)
    assert t.string_count() == len(flags)
    got = t.final_strings()
    assert got.dtype == bool and got.shape == (len(flags),)
    np.testing.assert_array_equal(got, final_rule(flags))
    if name == "hex":   # its two literal strings are chain parts
        lit = np.flatnonzero(flags & LITERAL)
        assert list(lit) == [9, 10] and not got[9] and not got[10]
    if name == "rx":
        assert not got.any()
    if name in ("lit", "short", "C"):
        assert got.any()


def test_final_strings_of_a_compiled_rules_file():
    """yr_amd_tables_load_yarc attaches the flags to host-only tables itself."""
    import gzip
    for name in ("hex", "lit", "C"):
        with gzip.open(os.path.join(GOLDEN, "yarc", "%s.yarc.gz" % name)) as f:
            t = yara_amd.Tables.from_yarc(f.read(), device=-1)
        np.testing.assert_array_equal(t.final_strings(),
                                      final_rule(np.load(tables_npz(name))["str_flags"]))


def _m(rows):
    a = np.zeros(len(rows), dtype=_lib.MATCH_REC_DTYPE)
    for k, r in enumerate(rows):
        a[k] = r
    return a


def test_merge_matches():
    # (offset, string, length, xor_key, pool_index), block-local offsets
    b0 = _m([(100, 0, 4, 0, 7), (900, 0, 8, 0x41, 7), (950, 2, 3, 0, 9)])
    # block 1 at base 800 overlaps block 0: absolute 900 and 950 again, with
    # another length / xor key (a match cut differently by the block's end)
    b1 = _m([(100, 0, 6, 0x42, 8), (300, 0, 4, 0, 7), (150, 2, 5, 0, 9), (10, 3, 2, 0, 1)])
    # block 2's base lies BEFORE block 1's matches: a smaller absolute offset
    b2 = _m([(5, 0, 4, 0, 7), (1, 3, 2, 0, 1)])
    got = yara_amd.merge_matches([(0, b0), (800, b1), (50, b2)])
    want = _m([(55, 0, 4, 0, 7), (100, 0, 4, 0, 7), (900, 0, 8, 0x41, 7), (1100, 0, 4, 0, 7),
               (950, 2, 3, 0, 9), (51, 3, 2, 0, 1), (810, 3, 2, 0, 1)])
    assert got.dtype == np.dtype(_lib.MATCH_REC_DTYPE)
    np.testing.assert_array_equal(got, want)
    # the inputs are left alone
    assert b1["offset"][0] == 100
    # one block: itself, sorted input unchanged
    np.testing.assert_array_equal(yara_amd.merge_matches([(0, b0)]), b0)
    # no blocks, and blocks without matches
    for empty in ([], [(0, _m([]))], [(0, _m([])), (4096, _m([]))]):
        e = yara_amd.merge_matches(empty)
        assert e.size == 0 and e.dtype == np.dtype(_lib.MATCH_REC_DTYPE)


def test_invalid_arguments():
    L = _lib.lib()
    INV = yara_amd.INVALID_ARGUMENT
    z = np.load(tables_npz("lit"))
    n = len(z["str_flags"])
    out = np.zeros(n + 1, np.uint8)
    op = out.ctypes.data_as(_lib._u8p)
    cnt = ctypes.c_uint32()
    # null tables
    assert L.yr_amd_tables_final_strings(None, op, n) == INV
    assert L.yr_amd_tables_string_count(None, ctypes.byref(cnt)) == INV
    assert L.yr_amd_tables_set_string_flags(None, None, 0) == INV
    # tables without string records
    bare = yara_amd.Tables.from_npz(tables_npz("lit"), device=-1)
    assert L.yr_amd_tables_final_strings(bare.handle, op, n) == INV
    assert L.yr_amd_tables_string_count(bare.handle, ctypes.byref(cnt)) == INV
    with pytest.raises(yara_amd.YaraAmdError) as e:
        bare.final_strings()
    assert e.value.code == INV
    # with them: the count must be the tables', the output not null
    t = yara_amd.Tables.from_npz(tables_npz("lit"), device=-1, strings=True)
    assert L.yr_amd_tables_final_strings(t.handle, op, n + 1) == INV
    assert L.yr_amd_tables_final_strings(t.handle, op, n - 1) == INV
    assert L.yr_amd_tables_final_strings(t.handle, None, n) == INV
    assert L.yr_amd_tables_string_count(t.handle, None) == INV
    assert L.yr_amd_tables_final_strings(t.handle, op, n) == yara_amd.SUCCESS
    # flags attach once, and need an array
    fl = np.ascontiguousarray(z["str_flags"], np.uint32)
    assert L.yr_amd_tables_set_string_flags(t.handle, fl.ctypes.data_as(_lib._u32p), n) == INV
    assert L.yr_amd_tables_set_string_flags(bare.handle, None, n) == INV
    # the device calls on null scanners
    assert L.yr_amd_match_device(None, 0, None, None, None, None) == INV
    assert L.yr_amd_scan_block_matches(None, None, 0, 0, None, None, None, None) == INV
