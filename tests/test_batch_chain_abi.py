"""The batch chain setting without a GPU: the symbols, their prototypes, the refusals that need
no scanner."""
import ctypes
import os
import re

import pytest

from yara_amd import _lib
from conftest import REPO


@pytest.mark.parametrize("name,prototype", [
    ("yr_amd_scanner_set_batch_chains",
     "int yr_amd_scanner_set_batch_chains(yr_amd_scanner* scanner, int enable);"),
    ("yr_amd_scanner_batch_chain_waves",
     "int yr_amd_scanner_batch_chain_waves(const yr_amd_scanner* scanner, uint32_t* waves);"),
])
def test_symbol(name, prototype):
    with open(os.path.join(REPO, "include", "yara_amd.h")) as f:
        header = f.read()
    assert hasattr(_lib.lib(), name) and name in _lib.PROTOTYPES
    assert prototype in header and len(re.findall(r"\bint %s\(" % name, header)) == 1
    assert _lib.PROTOTYPES[name][0] is ctypes.c_int and len(_lib.PROTOTYPES[name][1]) == 2


@pytest.mark.parametrize("value", [0, 1, 2, -1])
def test_null_scanner_is_refused(value):
    L = _lib.lib()
    assert L.yr_amd_scanner_set_batch_chains(None, value) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_scanner_batch_chain_waves(None, ctypes.byref(ctypes.c_uint32())) == \
        _lib.INVALID_ARGUMENT
