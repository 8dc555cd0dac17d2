"""CPU: the batch's loop setting (yr_amd_scanner_set_batch_loops) -- the symbol and its arguments.
(A scanner needs a device: the values 2 and -1 on a live scanner are in test_gpu_batch_loops.)"""
import pytest

import yara_amd
from yara_amd import _lib


@pytest.mark.parametrize("value", [1, 2, -1])
def test_symbol_and_arguments(value):
    proto = _lib.PROTOTYPES["yr_amd_scanner_set_batch_loops"]
    assert proto == _lib.PROTOTYPES["yr_amd_scanner_set_batch_alternations"]
    fn = _lib.lib().yr_amd_scanner_set_batch_loops
    assert fn.restype is proto[0] and fn.argtypes == proto[1]
    assert fn(None, value) == yara_amd.INVALID_ARGUMENT
    assert callable(yara_amd.Scanner.set_batch_loops)
