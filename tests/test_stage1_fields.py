"""Stage 1's shift amounts and block addresses, pair index by pair index.

The scan kernel's stage 1 (kernels.hip stage1, left_shifts, right_shifts,
pair_block_addr) takes the filter fields of a lane's 8 position pairs from
different places: even pairs from two context dwords through v_alignbit_b32 and
SDWA WORD_1 selects, odd pairs from one dword, the right windows of two pairs
from one v_perm.  A wrong field or address on ONE pair index loses the
candidates that end at particular lane bytes and nothing else, so these cases
plant strings at every residue mod 16 (test_gpu_parity.even_planted: across
lane, tile and segment edges too) and compare with the oracle -- for the pair
filter on config C (the existing planted cases cover B and E only), for the
1-byte-key kernels that run the same stage 1 (rx, short), and for every filter
form the diagnostic switches can force.
"""
import numpy as np
import pytest

import oracle
import yara_amd
from conftest import ALPHA, ref_tables, run_diag_child
from test_gpu_parity import dev_tables, even_planted

pytestmark = pytest.mark.gpu

STRIDES = [5, 7, 16, 33, 1021]
_DATA = {}
_REF = {}


def planted_c(stride):
    """Config C's strings every `stride` bytes in 2 MiB + 12,345 bytes (shared, read-only)."""
    if stride not in _DATA:
        d = even_planted("C", stride)
        d.setflags(write=False)
        _DATA[stride] = d
    return _DATA[stride]


def buffer_for(rules, stride):
    d = planted_c(stride)
    if rules == "short":   # the alphabet of `short`'s keys (test_ragged_sizes_vs_oracle)
        return np.frombuffer(ALPHA, np.uint8)[d % len(ALPHA)]
    return d


def reference(rules, stride):
    if (rules, stride) not in _REF:
        r = oracle.candidates(ref_tables(rules), buffer_for(rules, stride))
        r.setflags(write=False)
        _REF[(rules, stride)] = r
    return _REF[(rules, stride)]


@pytest.mark.parametrize("stride", STRIDES)
def test_pair_filter_config_c_every_lane_byte(stride):
    """Config C (the pair filter, scan_segments_kernel<0>): candidates equal the
    oracle's, and the reference itself ends candidates at each of the 16 lane
    bytes, so every pair index and both roles are exercised."""
    data = planted_c(stride)
    ref = reference("C", stride)
    per_lane_byte = np.bincount(((ref.astype(np.int64) - 1) % 16).astype(np.int64), minlength=16)
    print("stride %d: %d candidates, per lane byte %s" % (stride, len(ref), per_lane_byte.tolist()))
    assert per_lane_byte.min() >= 1
    assert len(ref) > data.size // stride // 8
    tab = dev_tables("C")
    assert tab.info()["filter_mode"] == 0
    pos, allp = yara_amd.Scanner(tab).candidates(data)
    assert not allp
    np.testing.assert_array_equal(pos, ref)


@pytest.mark.parametrize("rules", ["rx", "short"])
@pytest.mark.parametrize("stride", STRIDES)
def test_byte_key_kernels_same_stage1(rules, stride):
    """The 1-byte-key kernels run the same stage 1 before their own key tests."""
    data = buffer_for(rules, stride)
    ref = reference(rules, stride)
    assert len(ref) > 0
    pos, allp = yara_amd.Scanner(dev_tables(rules)).candidates(data)
    assert not allp
    np.testing.assert_array_equal(pos, ref)


def test_forced_filter_forms():
    """The forms the host can be forced into (diagnostic build, one child
    process): the plain and the hashed even filter on B and E, and the pair
    filter with B's, E's and C's windows; strides 5 and 1021."""
    code = (
        "import os, numpy as np, torch, yara_amd, oracle\n"
        "from conftest import ref_tables, tables_npz\n"
        "from test_gpu_parity import even_planted\n"
        "n = 0\n"
        "forms = (('YAMD_EVEN_FILTER', 'plain', 1), ('YAMD_EVEN_FILTER', 'hash', 2),\n"
        "         ('YAMD_PAIR_FILTER', '1', 0))\n"
        "for rules, use in (('B', forms), ('E', forms), ('C', forms[2:])):\n"
        "  for stride in (5, 1021):\n"
        "    data = even_planted(rules, stride)\n"
        "    ref = oracle.candidates(ref_tables(rules), data)\n"
        "    assert len(ref) > 0\n"
        "    for env, val, mode in use:\n"
        "      os.environ[env] = val\n"
        "      t = yara_amd.Tables.from_npz(tables_npz(rules), device=0)\n"
        "      del os.environ[env]\n"
        "      assert t.info()['filter_mode'] == mode, (rules, env, val)\n"
        "      got = yara_amd.Scanner(t).candidates(data)[0]\n"
        "      assert np.array_equal(got, ref), (rules, stride, mode)\n"
        "      n += 1\n"
        "print('forms ok', n)\n")
    assert "forms ok 14" in run_diag_child(code)
