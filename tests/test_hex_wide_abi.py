"""yr_amd_scanner_set_hex_wide without a GPU: the symbol and its refusals."""
import ctypes
import os
import re

import yara_amd
from yara_amd import _lib
from conftest import REPO

NAME = "yr_amd_scanner_set_hex_wide"


def test_symbol():
    with open(os.path.join(REPO, "include", "yara_amd.h")) as f:
        header = f.read()
    assert hasattr(_lib.lib(), NAME) and NAME in _lib.PROTOTYPES
    assert re.search(r"\bint %s\(yr_amd_scanner\* scanner, int enable\);" % NAME, header)
    assert callable(yara_amd.Scanner.set_hex_wide)


def test_null_scanner_and_values():
    for value in (0, 1, 2, -1):
        assert getattr(_lib.lib(), NAME)(ctypes.c_void_p(None), value) == yara_amd.INVALID_ARGUMENT
