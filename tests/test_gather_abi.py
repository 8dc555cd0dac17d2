"""Batches of buffers scattered in device memory, the part that needs no device:
the argument validation of yr_amd_batch_gather / yr_amd_scan_batch_gather_device
and of the Python wrappers, which refuse a bad buffer before the library is
called."""
import numpy as np
import pytest

import yara_amd
from yara_amd import _lib


def test_gather_calls_reject_a_null_scanner():
    L = _lib.lib()
    one = np.zeros(1, np.uint64)
    p = one.ctypes.data_as(_lib._u64p)
    assert L.yr_amd_batch_gather(None, None, 0, p, p, p, 1) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_batch_gather(None, None, 0, None, None, None, 0) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_scan_batch_gather_device(None, p, p, 1) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_scan_batch_gather_device(None, None, None, 0) == _lib.INVALID_ARGUMENT


def test_header_declares_the_gather_calls():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                          "yara_amd.h")).read()
    for name in ("yr_amd_batch_gather", "yr_amd_scan_batch_gather_device"):
        assert "int %s(" % name in h and name in _lib.PROTOTYPES


class FakeBuffer:
    """What the wrappers ask of a device buffer (a torch tensor's four methods)."""

    def __init__(self, size=8, element_size=1, contiguous=True):
        self._size, self._esize, self._contiguous = size, element_size, contiguous

    def data_ptr(self):
        return 0x1000

    def numel(self):
        return self._size

    def element_size(self):
        return self._esize

    def is_contiguous(self):
        return self._contiguous


class NoLibraryScanner(yara_amd.Scanner):
    """A scanner without a handle: any call that reached the library would fail
    on it with YaraAmdError (a null scanner), not with ValueError."""

    def __init__(self):
        self._h = None
        self._batch_n = 0


@pytest.mark.parametrize("call", ["batch_candidates_device", "batch_verify_calls_device"])
def test_wrappers_refuse_bad_buffers(call):
    sc = NoLibraryScanner()
    good = FakeBuffer()
    with pytest.raises(ValueError):
        getattr(sc, call)([good, FakeBuffer(element_size=2)])
    with pytest.raises(ValueError):
        getattr(sc, call)([FakeBuffer(contiguous=False), good])
    with pytest.raises(ValueError):
        getattr(sc, call)([(0x1000, 8), FakeBuffer(element_size=4, contiguous=False)])


def test_bases_length_mismatch_is_refused():
    sc = NoLibraryScanner()
    bufs = [FakeBuffer(), (0x2000, 4), FakeBuffer(size=0)]
    for bases in ([], [0], [0, 1], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            sc.batch_verify_calls_device(bufs, bases)
    # (the right length passes the wrapper's checks: the library is reached and
    # refuses the null scanner)
    with pytest.raises(yara_amd.YaraAmdError) as e:
        sc.batch_verify_calls_device(bufs, [0, 1, 2])
    assert e.value.code == _lib.INVALID_ARGUMENT


def test_wrappers_refuse_arrays_of_different_lengths():
    sc = NoLibraryScanner()
    with pytest.raises(ValueError):
        sc.batch_gather(0, 0, [0, 16], [0x1000], [4, 4])
    with pytest.raises(ValueError):
        sc.scan_batch_gather_device([0x1000, 0x2000], [4])
