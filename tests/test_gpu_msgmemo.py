"""The hash-point memo end to end (tb_msgmemo.h, k_msgmemo.hip,
tbls_msg_memo_configure / _stats / _clear): H(m) of a message a batch hashed
stays on the device, and later batches that sign the same bytes copy it from
there.

Verdicts are compared with the C oracle (oracle/c/bls_oracle.c: verify_each,
and the batch verdict as the conjunction of the per-set ones) and with the same
call at rows = 0; the counters with tests/msgmemo_model.py, a dictionary model
of the index's rules, fed with the stagings each call makes: one per call, and
a second one -- over the same sets, in the settle layout -- when a
tbls_batch_verify_each fails on a batch too small to settle from its own
workspace (up to 1,024 sets: the wave Miller loops leave no lines).

The memo is process state: the module configures it per test and turns it off
again at the end; settings read once per process run in child processes
(tests/msgmemo_cases.py).  One library device per process is assumed, as in
tests/test_gpu_pkcache.py: a batch always meets the device of the one before.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from oracle import c_oracle as C
from tests import msgmemo_cases as MC
from tests.msgmemo_model import Model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = MC.THREADS


@pytest.fixture(scope="module")
def W():
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import bls, native, synth

    native.lib()

    class world:
        pass

    w = world()
    w.bls, w.native, w.S = bls, native, synth
    yield w
    bls.msg_memo_configure(0)


def _oracle_each(pk, ms, sg):
    return C.verify_each([[p[48 * k : 48 * k + 48] for k in range(len(p) // 48)] for p in pk], ms, sg, threads=THREADS)


def _child(mode, **env):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("TBLS_MSG_MEMO", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.msgmemo_cases", mode], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_small_batch_every_rule(W):
    """rows = 4, 8 single-key sets.  Call 1 is cold: the four cacheable
    messages take the four rows, the 65-byte one is hashed and not learned;
    the batch fails (set 7) and is staged again to settle, where everything
    but the 65-byte message comes from the rows.  Call 2 repeats it.  Call 3
    brings five new messages to a full memo: a flush, four learned, the fifth
    hashed only."""
    S, native, bls = W.S, W.native, W.bls
    pk, (ms1, sg1), (ms3, sg3) = MC.small_batches(S)
    exp1, exp3 = _oracle_each(pk, ms1, sg1), _oracle_each(pk, ms3, sg3)
    assert exp1 == [True] * 7 + [False] and exp3 == [True] * 8
    r = S.random_multipliers(8)
    calls = [(ms1, sg1, exp1), (ms1, sg1, exp1), (ms3, sg3, exp3)]
    bls.msg_memo_configure(0)
    plain = [MC.each(S, native, pk, ms, sg, r) for ms, sg, _ in calls]
    assert bls.msg_memo_stats() == (0, 0, 0, 0)
    bls.msg_memo_configure(4)
    model = Model(4)
    for k, (ms, sg, exp) in enumerate(calls):
        got = MC.each(S, native, pk, ms, sg, r)
        assert got == (native.SUCCESS, int(all(exp)), exp), k
        assert got == plain[k], k
        model.shard(ms)
        if not all(exp):
            model.shard(ms)  # the second staging, to settle
        assert bls.msg_memo_stats() == model.stats(), k
    assert model.stats() == (7 + 14, 6 + 2 + 5, 1, 4)  # the model's figures, by hand
    # the counters reset, the rows in use stay; clear forgets the rows
    assert bls.msg_memo_stats(reset=True) == model.stats() and bls.msg_memo_stats() == (0, 0, 0, 4)
    bls.msg_memo_clear()
    assert bls.msg_memo_stats() == (0, 0, 0, 0)


def test_second_staging_of_a_failed_small_batch_hashes_nothing(W):
    """8 sets over 3 cacheable messages, one bad, rows = 4: the batch is below
    the wave-Miller limit, so it fails and is staged again in the settle
    layout; that second staging finds every message resident -- the messages
    hashed are the first staging's three, unchanged across the settle."""
    S, native, bls = W.S, W.native, W.bls
    pk, (ms1, sg1), _ = MC.small_batches(S)
    roots = [MC.msg(30), MC.msg(31), MC.msg(32)]
    ms = [roots[i % 3] for i in range(8)]
    sks = [S.interop_sk(900 + i) for i in range(8)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(8)]
    sg[2] = sg[5]  # key 5's signature (the same message, another key)
    exp = _oracle_each(pk, ms, sg)
    assert exp == [i != 2 for i in range(8)]
    bls.msg_memo_configure(4)
    before = native.stats()
    assert MC.each(S, native, pk, ms, sg, S.random_multipliers(8)) == (native.SUCCESS, 0, exp)
    after = native.stats()
    assert after["partials"] - before["partials"] == 2 and after["settled"] - before["settled"] == 1  # it was staged twice
    assert bls.msg_memo_stats() == (8, 3, 0, 3)


def test_above_the_byte_key_lookup_limit_and_grouped(W):
    """600 sets over 40 messages, rows = 64: tbls_batch_verify three times
    (40 hashed once, then 600 pairs from the rows per call), then
    tbls_batch_verify_each_grouped with TBLS_GROUP_FORCE and 2 bad sets: the
    grouped pass takes its 40 pairs from the rows and settles from its own
    workspace (no second staging)."""
    S, native, bls = W.S, W.native, W.bls
    n, m = 600, 40
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    roots = [S.bench_message(43, g) for g in range(m)]
    ms = [roots[(7 * i) % m] for i in range(n)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    assert _oracle_each(pk, ms, sg) == [True] * n
    r = S.random_multipliers(n)
    arr = S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [32] * n, b"".join(sg))
    bls.msg_memo_configure(64)
    model = Model(64)
    for k in range(3):
        assert arr.batch_verify(r) is True
        model.shard(ms)
        assert bls.msg_memo_stats() == model.stats() == (600 * k, 40, 0, 40)
    bad = [17, 599]
    sg2 = list(sg)
    sg2[17], sg2[599] = sg[18], bytes(96)
    exp = [i not in bad for i in range(n)]
    assert _oracle_each([pk[i] for i in bad], [ms[i] for i in bad], [sg2[i] for i in bad]) == [False, False]
    assert native.group_plan(n, m)[0] == 1  # grouped under TBLS_GROUP_FORCE only
    arr2 = S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [32] * n, b"".join(sg2))
    before = native.stats()
    assert arr2.batch_verify_each_grouped(r, force=True) == (False, exp)
    after = native.stats()
    assert after["partials"] - before["partials"] == 1 and after["settled"] - before["settled"] == 1
    model.shard(ms, per_set=False)
    assert bls.msg_memo_stats() == model.stats() == (1200 + 40, 40, 0, 40)
    bls.msg_memo_configure(0)
    assert arr2.batch_verify_each_grouped(r, force=True) == (False, exp)  # the same call without the memo


def test_split_kernels_and_a_settle_ready_batch(W):
    """2,304 sets, rows = 4,096.  Call 1: 2,304 distinct messages.  Call 2:
    the same, nothing hashed.  Call 3: every other message replaced by a new
    one, 3 bad sets, through tbls_batch_verify_each: 4,608 pairs run the split
    Miller kernels and the failed batch settles from its own lines (one
    staging)."""
    S, native, bls = W.S, W.native, W.bls
    n = 2304
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    ms = [S.bench_message(45, i) for i in range(n)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    r = S.random_multipliers(n)
    arr = S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [32] * n, b"".join(sg))
    assert all(C.verify_each([[k] for k in pk], ms, sg, threads=THREADS))
    bls.msg_memo_configure(4096)
    model = Model(4096)
    for k in range(2):
        assert arr.batch_verify(r) is True
        model.shard(ms)
        assert bls.msg_memo_stats() == model.stats() == (n * k, n, 0, n)
    ms3 = [S.bench_message(47, i) if i % 2 else ms[i] for i in range(n)]
    blob = S.sign_blob(sks, ms3)
    sg3 = [blob[96 * i : 96 * i + 96] for i in range(n)]
    sg3[0], sg3[1151], sg3[2303] = sg3[2], bytes(96), sg[2303]  # 2303 is odd: its old signature no longer fits
    exp = C.verify_each([[k] for k in pk], ms3, sg3, threads=THREADS)
    assert [i for i in range(n) if not exp[i]] == [0, 1151, 2303]
    before = native.stats()
    assert MC.each(S, native, pk, ms3, sg3, r) == (native.SUCCESS, 0, exp)
    after = native.stats()
    assert after["partials"] - before["partials"] == 1 and after["settled"] - before["settled"] == 1
    model.shard(ms3)
    assert bls.msg_memo_stats() == model.stats() == (n + n // 2, n + n // 2, 0, n + n // 2)


def test_a_shard_above_the_set_count_cutoff_bypasses_the_memo(W):
    """16,385 sets over 64 messages (TB_MEMO_SETS_MAX is 16,384), keys cyclic
    over 512: the shard is staged and hashed as without a memo -- nothing is
    counted and the rows of an earlier batch stay as they are; the 16,384 sets
    before the last one do resolve."""
    S, bls = W.S, W.bls
    n, m, K = 16385, 64, 512
    sks = [S.interop_sk(i) for i in range(K)]
    keys = S.pubkeys(sks)
    roots = [S.bench_message(49, g) for g in range(m)]
    ms = [roots[i % m] for i in range(n)]
    blob = S.sign_blob([sks[i % K] for i in range(n)], ms)
    pk = [keys[i % K] for i in range(n)]
    assert all(C.verify_each([[k] for k in pk[:256]], ms[:256], [blob[96 * i : 96 * i + 96] for i in range(256)], threads=THREADS))
    r = S.fast_multipliers(n)
    bls.msg_memo_configure(128)
    small = S.SetArray(b"".join(pk[:8]), [1] * 8, b"".join(ms[:8]), [32] * 8, blob[: 96 * 8])
    assert small.batch_verify(r[:8].copy()) is True and bls.msg_memo_stats() == (0, 8, 0, 8)
    arr = S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [32] * n, blob)
    assert arr.batch_verify(r, n_gpus=1) is True
    assert bls.msg_memo_stats() == (0, 8, 0, 8)
    at = S.SetArray(b"".join(pk[:-1]), [1] * (n - 1), b"".join(ms[:-1]), [32] * (n - 1), blob[: 96 * (n - 1)])
    assert at.batch_verify(r[: n - 1].copy(), n_gpus=1) is True
    assert bls.msg_memo_stats() == (8 * (16384 // 64), 8 + 56, 0, 64)


def test_per_set_pass(W):
    """tbls_fast_aggregate_verify_many on 8 sets of 3 keys over 2 messages,
    twice, with one bad set so that the per-set pass runs behind the batch;
    and the _idx form over a small table.  rows = 4."""
    S, native, bls = W.S, W.native, W.bls
    L = native.lib()
    keys, _, _ = S.multi_key(8, 3, first_key=700)
    roots = [MC.msg(50), MC.msg(51)]
    ms = [roots[i % 2] for i in range(8)]
    agg = [sum(S.interop_sk(700 + 3 * s + k) for k in range(3)) % S.R_ORDER for s in range(8)]
    blob = S.sign_blob(agg, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(8)]
    sg[5] = sg[3]
    exp = C.verify_each(keys, ms, sg, threads=THREADS)
    assert exp == [i != 5 for i in range(8)]
    arr = S.SetArray.from_lists(keys, ms, sg)
    bls.msg_memo_configure(0)
    assert arr.fast_aggregate_verify_many() == exp
    bls.msg_memo_configure(4)
    model = Model(4)
    for k in range(2):
        assert arr.fast_aggregate_verify_many() == exp
        model.shard(ms)  # the randomized batch, which fails
        model.shard(ms)  # the per-set pass
        assert bls.msg_memo_stats() == model.stats() == (8 + 16 * k, 2, 0, 2)
    # by table index: the same sets, their 24 keys as a table
    table = [k for ks in keys for k in ks]
    native.check(L.tbls_pk_table_load(b"".join(table), len(table), None), "pk_table_load")
    try:
        idx = (ctypes.c_uint32 * 24)(*range(24))
        mbuf, sbuf = ctypes.create_string_buffer(b"".join(ms), 32 * 8), ctypes.create_string_buffer(b"".join(sg), 96 * 8)
        sets = (native.TblsSetIdx * 8)()
        for i in range(8):
            sets[i].key_idx = ctypes.addressof(idx) + 12 * i
            sets[i].n_pks = 3
            sets[i].msg = ctypes.addressof(mbuf) + 32 * i
            sets[i].msg_len = 32
            sets[i].sig = ctypes.addressof(sbuf) + 96 * i
        out = (ctypes.c_int * 8)()
        native.check(L.tbls_fast_aggregate_verify_many_idx(sets, 8, out), "fast_aggregate_verify_many_idx")
        assert [v == 1 for v in out] == exp
        model.shard(ms)
        model.shard(ms)
        assert bls.msg_memo_stats() == model.stats() == (40, 2, 0, 2)
    finally:
        native.check(L.tbls_pk_table_clear(), "pk_table_clear")


def test_two_library_devices(W):
    """Two library devices over the one GPU: each shard of 300 sets holds all
    40 messages and uses its own device's memo -- 2 x 40 hashed by the first
    call, 600 pairs from the rows in every later staging."""
    got = _child("two_devices", TBLS_SHARD_MIN="300", TBLS_MSG_MEMO="64")
    assert got["devices"] == 2 and [c["n_devices"] for c in got["calls"]] == [2, 2]
    assert [c["ok"] for c in got["calls"]] == [True, True]
    assert [c["memo"] for c in got["calls"]] == [[0, 80, 0, 80], [600, 80, 0, 80]]
    e = got["each"]
    assert (e["rc"], e["ok"]) == (0, 0) and e["failed"] == e["expected"] == [10, 590]
    assert e["memo"] == [600 + 2 * 600, 80, 0, 80]  # the failed batch's two shards are staged again to settle


def test_off_switch(W):
    """Without TBLS_MSG_MEMO, and after tbls_msg_memo_configure(0), nothing is
    counted, the verdicts are the same and the library runs the same passes."""
    S = W.S
    pk, (ms1, sg1), (ms3, sg3) = MC.small_batches(S)
    exp1, exp3 = _oracle_each(pk, ms1, sg1), _oracle_each(pk, ms3, sg3)
    want = [[0, int(all(e)), e] for e in (exp1, exp1, exp3)]
    never, configured = _child("off_env"), _child("off_configured")
    assert configured["used_before"][3] == 4  # the memo was in use before it was turned off
    for got in (never, configured):
        assert got["calls"] == want
        assert got["memo"] == [0, 0, 0, 0]
    assert never["stats"] == configured["stats"]
    assert never["stats"]["partials"] == 5 and never["stats"]["settled"] == 2  # two failed batches staged twice, one valid one
