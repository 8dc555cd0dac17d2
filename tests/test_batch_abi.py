"""Batched scans, the part of the C ABI that needs no device: the arena layout
(yr_amd_batch_layout) and the argument validation of the batch calls."""
import ctypes

import numpy as np
import pytest

import yara_amd
from yara_amd import _lib

MAX_BUFFERS = 0x7FFFFFFF   # YR_AMD_BATCH_MAX_BUFFERS


def _check_layout(sizes):
    starts, arena = yara_amd.batch_layout(sizes)
    sizes = np.asarray(sizes, np.uint64)
    assert starts.dtype == np.uint64 and starts.shape == sizes.shape
    assert np.all(starts % 16 == 0)
    if len(sizes):
        assert starts[0] == 0
        ends = starts + sizes
        assert np.all(starts[1:] >= ends[:-1])            # ascending, no overlap
        assert np.all(starts[1:] - ends[:-1] < 16)        # gaps: alignment only
        assert arena == ends[-1]
    else:
        assert arena == 0
    return starts, arena


@pytest.mark.parametrize("sizes", [
    [], [0], [0, 0, 0], [1], [16], [17, 0, 0, 5], [0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025],
    [4096, 4097, 4095, 70001, 0],
])
def test_layout(sizes):
    _check_layout(sizes)


def test_layout_empty_buffers_share_the_next_start():
    starts, arena = _check_layout([5, 0, 0, 7])
    assert list(starts) == [0, 16, 16, 16] and arena == 23


def test_layout_many():
    rng = np.random.default_rng(3)
    _check_layout(rng.integers(0, 65, 70000))


def test_layout_rejects_overflow_and_too_many():
    L = _lib.lib()
    sizes = np.array([2**64 - 8, 16], np.uint64)
    starts = np.zeros(2, np.uint64)
    arena = ctypes.c_uint64()
    p = lambda a: a.ctypes.data_as(_lib._u64p)
    assert L.yr_amd_batch_layout(p(sizes), 2, p(starts), ctypes.byref(arena)) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_batch_layout(p(sizes), MAX_BUFFERS + 1, p(starts),
                                 ctypes.byref(arena)) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_batch_layout(None, 1, p(starts), ctypes.byref(arena)) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_batch_layout(p(sizes), 1, None, ctypes.byref(arena)) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_batch_layout(None, 0, None, None) == _lib.SUCCESS


def test_batch_calls_reject_a_null_scanner():
    L = _lib.lib()
    one = np.zeros(1, np.uint64)
    p = one.ctypes.data_as(_lib._u64p)
    assert L.yr_amd_scan_batch_device(None, None, 0, p, p, 1) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_scan_batch_result(None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_verify_batch_device(None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.yr_amd_scan_batch_verified(None, None, None, None, 0, None, None) == _lib.INVALID_ARGUMENT


def test_header_documents_the_limits():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                          "yara_amd.h")).read()
    assert "#define YR_AMD_BATCH_MAX_BUFFERS 0x7FFFFFFFull" in h   # (>= 2^20 buffers)
    assert MAX_BUFFERS >= 1 << 20
