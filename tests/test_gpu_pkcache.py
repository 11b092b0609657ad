"""The learned key cache (tb_pkindex.h pkx_cache, k_pkindex.hip
k_pk_lookup + k_pk_decompress_list + k_pk_learn; tbls_pk_cache_stats,
tbls_pk_cache_clear): byte keys that a key stage decompressed and found valid
stay on the device, and the next batches take them from there.

Verdicts are compared with the C oracle (oracle/c/bls_oracle.c) on the same
bytes, and the counters with exact values derived from the batch's layout
(tests/pklookup_cases.py: 600 single-key sets, the smallest size above the
one-kernel key stage that looks nothing up; 3 x 40 keys) and from the key
stages each call runs (tests/test_gpu_pklookup.py's docstring: one per call,
two for a tbls_batch_verify_each that fails and is staged again to settle).

The cache is process state: every case starts from tbls_pk_cache_clear, and
the settings that are read once per process run in child processes.
"""

import json
import os
import subprocess
import sys

import pytest

from oracle import c_oracle as C
from tests import pkcache_cases as PC
from tests import pklookup_cases as K

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def W():
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import bls, native

    native.lib()
    bls.ValidatorKeyTable.lookup_stats(reset=True)
    native.lib().tbls_pk_table_clear()
    w = K.World()
    w.bls, w.native = bls, native
    pk, ms, sg = w.single
    w.exp_single = C.verify_each([[p] for p in pk], ms, sg, threads=THREADS)
    assert [p for p, v in enumerate(w.exp_single) if not v] == [K.P_INF, K.P_BAD, K.P_TAMPER]
    # the batch's valid keys (every key but the infinity key and BAD_PK), and the distinct ones among them
    valid = [k for p, k in enumerate(pk) if p not in (K.P_INF, K.P_BAD)]
    w.V, w.D = len(valid), len(set(valid))
    assert w.V == 598 and 77 < w.D < w.V  # table keys repeat (set p carries table key 7 p mod 300)
    yield w
    native.lib().tbls_pk_table_clear()
    bls.pk_cache_clear()


@pytest.fixture(autouse=True)
def cold(W):
    W.native.lib().tbls_pk_table_clear()
    W.bls.pk_cache_clear()
    assert W.bls.pk_cache_stats() == (0, 0, 0, 0)


def _child(mode, **env):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "-m", "tests.pkcache_cases", mode], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _verdicts(W, calls):
    for r in calls:
        if "ok" in r:
            assert r["ok"] is False  # the batch holds the infinity key, BAD_PK and a tampered signature
        if "each" in r:
            assert r["each"] == W.exp_single


def test_cold_then_warm(W):
    """No table.  The first key stage finds nothing and learns the distinct
    valid keys; every later stage takes the 598 valid keys from the cache and
    decompresses the infinity key and BAD_PK again (they fail their sets as
    before: the verdicts equal the oracle's in every call).  The table's
    counters stay 0."""
    V, D = W.V, W.D
    first = PC.run_calls(W, W.single)
    _verdicts(W, first)
    hits, learned, refused, rows = first[0]["cache"]
    assert (hits, learned, refused) == (0, D, 0) and D <= rows <= V  # a key the batch holds twice may leave a row unused
    assert first[1]["cache"] == [V, 0, 0, rows]
    assert first[2]["cache"] == [2 * V, 0, 0, rows]  # the failed batch is staged again to settle: two key stages
    second = PC.run_calls(W, W.single)
    _verdicts(W, second)
    assert [r["cache"] for r in second] == [[V, 0, 0, rows], [V, 0, 0, rows], [2 * V, 0, 0, rows]]
    assert all(r["lookup"] == [0, 0] for r in first + second)


def test_multi_key_sets(W):
    """3 sets x 40 keys through tbls_fast_aggregate_verify_many and
    tbls_batch_verify: 120 distinct valid keys learned by the first key stage,
    all hits afterwards, verdicts equal the oracle's."""
    keys, ms, sg = W.multi
    assert len({k for ks in keys for k in ks}) == 120
    exp = C.verify_each(keys, ms, sg, threads=THREADS)
    assert exp == [True] * 3
    arr = W.S.SetArray.from_lists(keys, ms, sg)
    assert arr.fast_aggregate_verify_many() == exp
    assert PC.cache_stats() == [0, 120, 0, 120]
    assert arr.batch_verify(K.rands(W, 3)) is True
    assert PC.cache_stats() == [120, 0, 0, 120]
    assert arr.fast_aggregate_verify_many() == exp
    assert PC.cache_stats() == [120, 0, 0, 120]


def test_dev_batch_partial_records(W):
    """tbls_dev_batch_partial's 580-byte record is byte-equal cold, warm, and
    in a child process with TBLS_PK_CACHE=0 (whose counters stay 0)."""
    part = PC.DevPartial(W, W.single_valid)
    valid = W.single_valid[0]
    rec_cold, ok_cold = part()
    assert ok_cold == 1 and PC.cache_stats()[:3] == [0, len(set(valid)), 0]
    rec_warm, ok_warm = part()
    assert ok_warm == 1 and PC.cache_stats()[:3] == [len(valid), 0, 0]
    assert rec_warm == rec_cold
    got = _child("record", TBLS_PK_CACHE="0")
    assert [r["cache"] for r in got["records"]] == [[0, 0, 0, 0]] * 2
    assert [(r["rec"], r["ok"]) for r in got["records"]] == [(rec_cold, 1)] * 2


def test_eight_distinct_keys(W):
    """600 sets over 8 distinct keys: concurrent appenders of equal bytes end
    as one entry each -- exactly 8 keys learned, and the second call is all
    hits."""
    batch = PC.eight_key_batch(W)
    pk, ms, sg = batch
    assert len(set(pk)) == 8
    assert C.batch_verify(pk, ms, sg, K.rands(W, K.N_SINGLE), threads=THREADS) is True
    calls = PC.run_calls(W, batch, calls=("batch_verify", "batch_verify", "verify_each"))
    assert calls[0]["ok"] is True and calls[1]["ok"] is True and calls[2]["each"] == [True] * K.N_SINGLE
    hits, learned, refused, rows = calls[0]["cache"]
    assert (hits, learned, refused) == (0, 8, 0) and 8 <= rows <= K.N_SINGLE
    assert calls[1]["cache"] == [K.N_SINGLE, 0, 0, rows] and calls[2]["cache"] == [K.N_SINGLE, 0, 0, rows]


def test_small_cache_in_child(W):
    """TBLS_PK_CACHE_KEYS=64: the first key stage takes all 64 rows (the batch
    has more distinct valid keys than that), learns at most 64 keys and
    refuses the others; from then on nothing is learned, every valid key is
    either a hit or refused again (and decompressed), and every call is
    correct."""
    got = _child("small", TBLS_PK_CACHE_KEYS="64")
    calls = got["rounds"][0] + got["rounds"][1]
    _verdicts(W, calls)
    hits, learned, refused, rows = calls[0]["cache"]
    assert hits == 0 and 0 < learned <= 64 and rows == 64 and refused >= W.D - 64
    for r, stages in zip(calls[1:], [1, 2, 1, 1, 2]):
        h, l, f, rows = r["cache"]
        assert rows == 64 and l == 0 and f > 0
        assert stages * learned <= h and h + f == stages * W.V


def test_table_first_then_cache(W):
    """With TABLE loaded the table's counters equal the exact counts of
    tests/test_gpu_pklookup.py on both calls (523 hits, 77 misses), the cache
    learns the 77 keys the table lacks, and on the second call its hits are
    exactly those 77: keys the table holds never reach the cache."""
    t = W.bls.ValidatorKeyTable(W.TABLE)
    assert t.lookup_stats() == (0, 0)
    assert W.hits(W.single[0], W.TABLE) == (523, 77)
    calls = PC.run_calls(W, W.single, calls=("batch_verify", "batch_verify", "verify_each"))
    _verdicts(W, calls)
    assert [r["lookup"] for r in calls] == [[523, 77]] * 3
    assert calls[0]["cache"] == [0, 77, 0, 77]
    assert calls[1]["cache"] == [77, 0, 0, 77] and calls[2]["cache"] == [77, 0, 0, 77]
    # the cache outlives the table; what the table held was never learned
    t.clear()
    after = PC.run_calls(W, W.single, calls=("batch_verify", "batch_verify"))
    _verdicts(W, after)
    hits, learned, refused, rows = after[0]["cache"]
    assert (hits, learned, refused) == (77, W.D - 77, 0)
    assert after[1]["cache"] == [W.V, 0, 0, rows] and [r["lookup"] for r in after] == [[0, 0]] * 2


def test_clear_makes_the_next_call_cold(W):
    first = PC.run_calls(W, W.single, calls=("batch_verify", "batch_verify"))
    assert first[0]["cache"][:3] == [0, W.D, 0] and first[1]["cache"][:3] == [W.V, 0, 0]
    W.bls.pk_cache_clear()
    assert W.bls.pk_cache_stats() == (0, 0, 0, 0)
    again = PC.run_calls(W, W.single, calls=("batch_verify", "batch_verify"))
    _verdicts(W, again)
    assert again[0]["cache"][:3] == [0, W.D, 0] and again[1]["cache"][:3] == [W.V, 0, 0]


def test_two_library_devices(W):
    """Two library devices over the one GPU (TBLS_INIT_SHARE_DEVICES), 1,200
    sets (the 600 keys twice) sharded 600 + 600: each device learns the
    distinct valid keys of its own shard, so the summed counters are twice one
    device's."""
    got = _child("two_devices", TBLS_SHARD_MIN="600")
    assert got["devices"] == 2 and [c["n_devices"] for c in got["calls"]] == [2, 2]
    assert [c["ok"] for c in got["calls"]] == [False, False]
    hits, learned, refused, rows = got["calls"][0]["cache"]
    assert (hits, learned, refused) == (0, 2 * W.D, 0) and 2 * W.D <= rows <= 2 * W.V
    assert got["calls"][1]["cache"] == [2 * W.V, 0, 0, rows]
    batch = W.single_times(2)
    assert got["each"] == C.verify_each([[p] for p in batch[0]], batch[1], batch[2], threads=THREADS)


def test_lookup_off_in_child(W):
    """TBLS_PK_LOOKUP=0: no lookup and no cache -- every counter stays 0 and the verdicts are the same."""
    got = _child("lookup_off", TBLS_PK_LOOKUP="0")
    calls = got["rounds"][0] + got["rounds"][1]
    _verdicts(W, calls)
    assert all(r["cache"] == [0, 0, 0, 0] and r["lookup"] == [0, 0] for r in calls)
