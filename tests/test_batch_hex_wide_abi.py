"""yr_amd_scanner_set_batch_hex_wide without a GPU: the symbol and the refusal of NULL.
(A scanner needs a device: that 0 and 1 are accepted and 2 is refused on a live scanner
is test_gpu_batch_hex_wide.py's.)"""
import ctypes
import os
import re

import yara_amd
from yara_amd import _lib
from conftest import REPO

NAME = "yr_amd_scanner_set_batch_hex_wide"


def test_symbol():
    with open(os.path.join(REPO, "include", "yara_amd.h")) as f:
        header = f.read()
    assert hasattr(_lib.lib(), NAME) and NAME in _lib.PROTOTYPES
    assert _lib.PROTOTYPES[NAME] == _lib.PROTOTYPES["yr_amd_scanner_set_hex_wide"]
    assert re.search(r"\bint %s\(yr_amd_scanner\* scanner, int enable\);" % NAME, header)
    assert callable(yara_amd.Scanner.set_batch_hex_wide)


def test_null_scanner_is_refused_for_any_value():
    for value in (0, 1, 2, -1):
        assert getattr(_lib.lib(), NAME)(ctypes.c_void_p(None), value) == yara_amd.INVALID_ARGUMENT
