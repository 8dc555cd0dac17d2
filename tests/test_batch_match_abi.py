"""The batch match stage's ABI without a GPU: the two calls exist in the
library, in the ctypes table and in the header, and refuse a null scanner."""
import os
import re

import yara_amd
from yara_amd import _lib

NAMES = ("yr_amd_match_batch_device", "yr_amd_scan_batch_matches")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "yara_amd.h")


def test_null_scanner():
    L = _lib.lib()
    INV = yara_amd.INVALID_ARGUMENT
    assert L.yr_amd_match_batch_device(None, None, None, None, None, None) == INV
    assert L.yr_amd_scan_batch_matches(None, None, None, None, 0, None, None, None, None) == INV


def test_lib_declares_both():
    for name in NAMES:
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is _lib._int
        assert len(argtypes) == (6 if name == NAMES[0] else 9)
        assert getattr(_lib.lib(), name).argtypes == argtypes


def test_header_declares_both():
    with open(HEADER) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    # the arguments the issue names, in order
    decl = text[text.index("int yr_amd_match_batch_device("):]
    decl = decl[:decl.index(");")]
    assert [w for w in ("bases", "d_matches", "match_off", "d_rest", "rest_off")
            if w in decl] == ["bases", "d_matches", "match_off", "d_rest", "rest_off"]
