"""yr_gpu_scanner_scan_mem_batch against stock libyara, buffer by buffer.

oracle/_ref/batch_check (integration/batch_check.c) cuts a data file into
pieces, scans each piece with stock yr_scanner_scan_mem and the whole list with
yr_gpu_scanner_scan_mem_batch, and compares per-piece matches ({string, offset,
length, xor key}), rule reports and the order of every callback.  The checker
needs the reference headers at build time and lives in oracle/_ref/.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import gen_rules
import oracle
import planted
from conftest import ALPHA, GOLDEN, REPO, ref_tables

pytestmark = pytest.mark.gpu

CHECK = os.path.join(REPO, "oracle", "_ref", "batch_check")
needs_check = pytest.mark.skipif(not os.path.exists(CHECK),
                                 reason="oracle/_ref/batch_check not built "
                                        "(needs the reference headers at build time)")

ERROR_CALLBACK_ERROR = 28


def _rules_file(tmp_path, name):
    p = tmp_path / ("%s.yar" % name)
    if name in ("short", "root", "lit", "hex", "rx"):
        p.write_text(open(os.path.join(GOLDEN, "rules", name + ".yar")).read())
    else:
        p.write_text(gen_rules.gen(name))
    return str(p)


def _data(name):
    if name == "C":
        return planted.planted_buffer(oracle.xorshift, gen_rules.gen("C"), 1 << 20, 3)
    if name == "lit":
        return planted.lit_buffer(oracle.xorshift, 1 << 20, 13)
    if name == "hex":
        return planted.hex_buffer(oracle.xorshift, 1 << 20, 17)
    if name == "rx":
        return planted.rx_buffer(oracle.xorshift, 1 << 19, 19)
    size = 4096 if name == "root" else 1 << 18
    x = oracle.xorshift(size, 5)
    return np.frombuffer(ALPHA, np.uint8)[x % len(ALPHA)]


def _cuts(name, data, n_keys=8):
    """Cuts at P - 3 .. P + 1 around candidates P of the whole buffer (keys
    straddle cuts, end at a buffer's end, leave 1..3 bytes to the next one)."""
    P = oracle.candidates(ref_tables(name), data).astype(np.int64)
    P = P[(P > 8) & (P < len(data) - 8)]
    cuts = set()
    for p in P[np.linspace(0, len(P) - 1, n_keys).astype(int)]:
        cuts.update(int(p) + d for d in range(-3, 2))
    return sorted(cuts)


def _run(tmp_path, name, cuts=None, **env):
    data = _data(name)
    if cuts is None:
        cuts = _cuts(name, data)
    d = tmp_path / "d.bin"
    np.asarray(data, dtype=np.uint8).tofile(str(d))
    c = tmp_path / "cuts.txt"
    c.write_text("".join("%d\n" % x for x in cuts))
    r = subprocess.run([CHECK, _rules_file(tmp_path, name), str(d), str(c)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, **env))
    assert r.stdout, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["pieces"] == len(cuts) + 1
    return r.returncode, res


def _all_equal(rc, res):
    assert res["rc_stock"] == 0 and res["rc_gpu"] == 0, res
    assert res["done_stock"] == res["pieces"] and res["done_gpu"] == res["pieces"], res
    assert res["same_matches"] and res["same_events"], res
    assert res["events_stock"] > res["pieces"], res
    assert rc == 0


@needs_check
@pytest.mark.parametrize("name", ["C", "lit", "hex", "rx", "short"])
def test_batch_equals_stock_per_buffer(tmp_path, name):
    rc, res = _run(tmp_path, name)
    _all_equal(rc, res)
    assert res["arenas"] >= 1, res
    if name != "short":   # the planted cases
        assert res["matches_stock"] > 0 and res["rules_matching"] > 0, res


@needs_check
def test_root_accepting_rules_fall_back(tmp_path):
    rc, res = _run(tmp_path, "root", cuts=[0, 1, 5, 100, 101, 4000])
    _all_equal(rc, res)
    assert res["arenas"] == 0, res   # (no batch pre-verification on such rules)


@needs_check
def test_preverify_off_falls_back(tmp_path):
    rc, res = _run(tmp_path, "lit", BATCH_PREVERIFY="0")
    _all_equal(rc, res)
    assert res["arenas"] == 0, res


@needs_check
def test_several_arenas_and_oversized_buffers(tmp_path):
    """An arena limit forced small: the list spans several arenas, and a piece
    larger than the limit takes the per-buffer path in its place."""
    data = _data("lit")
    cuts = sorted(set(_cuts("lit", data) + list(range(4096, 400000, 9973)) + [700000]))
    sizes = np.diff([0] + cuts + [len(data)])
    assert sizes.max() > 65536 > sizes.min()
    rc, res = _run(tmp_path, "lit", cuts=cuts, BATCH_ARENA="65536")
    _all_equal(rc, res)
    assert res["arenas"] >= 4, res
    assert res["matches_stock"] > 0, res


@needs_check
def test_callback_error_in_the_middle_stops_the_batch(tmp_path):
    data = _data("lit")
    cuts = _cuts("lit", data)
    k = len(cuts) // 2
    rc, res = _run(tmp_path, "lit", cuts=cuts, BATCH_ERROR_AT=str(k))
    assert res["rc_stock"] == ERROR_CALLBACK_ERROR and res["rc_gpu"] == ERROR_CALLBACK_ERROR, res
    assert res["done_stock"] == k and res["done_gpu"] == k, res
    assert res["same_matches"] and res["same_events"], res
    assert rc == 0
