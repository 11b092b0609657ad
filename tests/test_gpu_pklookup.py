"""Byte-keyed batches resolve known keys from the resident key table's index
(tb_pkindex.h, k_pkindex.hip: k_pk_lookup + k_pk_decompress_list in the key
stage of launch_partial and run_each; tbls_pk_table_resolve,
tbls_pk_lookup_stats, tbls_pk_table_clear).

Verdicts are compared with the C oracle (oracle/c/bls_oracle.c) on the same
bytes, resolve with a Python dict over the table's bytes, and the lookup
counters with the exact hit and miss counts of each call, derived from the
batch's layout (tests/pklookup_cases.py) and from the key stages the call runs:

 * tbls_batch_verify and tbls_verify_each run one key stage over the batch's
   keys;
 * tbls_batch_verify_each runs one, and when the batch fails a second one: a
   600-set batch is 1,200 pairs, which run the one-wave Miller loops (no
   lines to settle from, tb_plan.h settle_ready), so the failed batch is
   staged again in the settle layout, key stage included;
 * tbls_fast_aggregate_verify_many runs the randomized batch's key stage, and
   when that batch fails the per-set pass's as well.

The table is process state: the module's finaliser clears it, and the
settings that are read once per process run in child processes.
"""

import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

from oracle import c_oracle as C
from tests import pklookup_cases as K

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def W():
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import bls, native

    native.lib()
    w = K.World()
    w.bls, w.native = bls, native
    pk, ms, sg = w.single
    w.exp_single = C.verify_each([[p] for p in pk], ms, sg, threads=THREADS)
    yield w
    native.lib().tbls_pk_table_clear()  # later test files start without a table


def _load(W, keys):
    t = W.bls.ValidatorKeyTable(keys)
    assert t.lookup_stats() == (0, 0)  # a load zeroes the counters
    return t


def _child(args, **env):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "-m", "tests.pklookup_cases"] + args, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _check_single(W, got, table_keys, batch=None, exp=None, stages=1):
    """The three calls' verdicts against the oracle's, and their counters
    against `stages` key stages per call (per shard) over the batch's keys."""
    pk = (batch or W.single)[0]
    exp = exp if exp is not None else W.exp_single
    h, m = W.hits(pk, table_keys)
    assert h + m == len(pk)
    failed = not all(exp)
    assert got["batch_verify"]["ok"] == all(exp)
    assert got["batch_verify"]["stats"] == [stages * h, stages * m]
    if "verify_each" in got:
        assert got["verify_each"]["each"] == exp
        assert got["verify_each"]["stats"] == [stages * h, stages * m]
    assert got["batch_verify_each"]["ok"] == all(exp) and got["batch_verify_each"]["each"] == exp
    k = 2 if failed else 1  # the failed batch is staged again to settle (module docstring)
    assert got["batch_verify_each"]["stats"] == [stages * k * h, stages * k * m]
    return h, m


# ---------------------------------------------------------------------------
def test_resolve(W):
    """Every table key in shuffled order, 70 keys outside the table, a table
    key with its last byte changed and one with only a flag bit changed: each
    answer points at equal bytes, or is 0xFFFFFFFF exactly where the table has
    no such bytes.  Resolving counts nothing."""
    t = _load(W, W.TABLE)
    assert t.size == 304 and t.codes[:300] == [0] * 300 and all(t.codes[300:303]) and t.codes[303] == 0
    where = {}
    for i, k in enumerate(W.TABLE):
        where.setdefault(k, []).append(i)
    assert where[W.TABLE[0]] == [0, 303]
    last = bytearray(W.TABLE[5])
    last[47] ^= 1
    flag = bytearray(W.TABLE[6])
    flag[0] ^= 0x20
    q = list(W.TABLE)
    random.Random(7).shuffle(q)
    q += W.pk_out[:70] + [bytes(last), bytes(flag)]
    got = t.resolve(q)
    assert len(got) == len(q)
    for k, i in zip(q, got):
        if k in where:
            assert i in where[k] and W.TABLE[i] == k
        else:
            assert i == MISS
    assert got[-2:] == [MISS, MISS] and got[304:374] == [MISS] * 70
    assert t.resolve([]) == []
    assert t.resolve([W.TABLE[301]]) == [301]  # an invalid key is still a table key
    assert t.lookup_stats() == (0, 0)


def test_single_key_batch(W):
    """600 single-key sets, 77 of them with keys outside the table (first,
    last, every 8th), the infinity key and BAD_PK as hits, one tampered
    signature: tbls_batch_verify, tbls_verify_each and tbls_batch_verify_each
    (which fails and settles) equal the oracle, and the counters equal the
    layout's counts.  Then with a table that lacks the two invalid keys, which
    are then misses, and with an all-valid batch, which passes."""
    assert W.native.acc_plan(K.N_SINGLE)[2] == 0  # the wave Miller loops: a failed batch is staged again
    exp = W.exp_single
    assert [p for p, v in enumerate(exp) if not v] == [K.P_INF, K.P_BAD, K.P_TAMPER]
    _load(W, W.TABLE)
    assert _check_single(W, K.run_single(W, W.single), W.TABLE) == (523, 77)
    _load(W, W.TABLE_LACKING)
    assert _check_single(W, K.run_single(W, W.single), W.TABLE_LACKING) == (521, 79)
    # all valid: the randomized batch accepts
    pk, ms, sg = W.single_valid
    assert C.batch_verify(pk, ms, sg, K.rands(W, K.N_SINGLE), threads=THREADS) is True
    _load(W, W.TABLE)
    assert _check_single(W, K.run_single(W, W.single_valid), W.TABLE, batch=W.single_valid, exp=[True] * K.N_SINGLE) == (523, 77)


def test_below_the_lookup(W):
    """Out of scope and unchanged: a single-key batch of up to 512 sets decodes
    its keys in its one key kernel (k_keys_coop) and counts nothing."""
    _load(W, W.TABLE)
    n = 512
    got = K.run_single(W, W.single, n)
    assert got["batch_verify"]["ok"] is False and got["batch_verify"]["stats"] == [0, 0]
    assert got["batch_verify_each"]["each"] == W.exp_single[:n]
    assert got["verify_each"]["each"] == W.exp_single[:n]
    h, m = W.hits(W.single[0][:n], W.TABLE)
    assert got["verify_each"]["stats"] == [h, m]  # the per-set pass decompresses at every size: it looks up


def test_multi_key(W):
    """3 sets x 40 keys -- all hits, all misses, mixed -- through
    tbls_fast_aggregate_verify_many and tbls_batch_verify: verdicts equal the
    oracle, counts exact; then with a tampered signature, where the per-set
    pass runs a second key stage."""
    keys, ms, sg = W.multi
    flat = [k for ks in keys for k in ks]
    _load(W, W.TABLE)
    h, m = W.hits(flat, W.TABLE)
    assert (h, m) == (60, 60)
    exp = C.verify_each(keys, ms, sg, threads=THREADS)
    assert exp == [True] * 3
    assert C.batch_verify_sets(keys, ms, sg, K.rands(W, 3), threads=THREADS) is True
    got = K.run_multi(W, W.multi)
    assert got["fast_aggregate_verify_many"] == {"each": exp, "stats": [h, m]}
    assert got["batch_verify"] == {"ok": True, "stats": [h, m]}
    bad = (keys, ms, [sg[0], sg[0], sg[2]])
    exp = C.verify_each(*bad, threads=THREADS)
    assert exp == [True, False, True]
    got = K.run_multi(W, bad)
    assert got["fast_aggregate_verify_many"] == {"each": exp, "stats": [2 * h, 2 * m]}
    assert got["batch_verify"] == {"ok": False, "stats": [h, m]}


def test_state_clear_and_reload(W):
    """After clear() the same batches give the same verdicts and the counters
    stay 0, and resolve has no table; after loading a table of other keys, the
    keys the first table knew are misses."""
    t = _load(W, W.TABLE)
    with_table = K.run_single(W, W.single)
    t.clear()
    L = W.native.lib()
    assert L.tbls_pk_table_size() == 0
    idx = (ctypes.c_uint32 * 1)()
    assert L.tbls_pk_table_resolve(W.TABLE[0], 1, idx) == W.native.BAD_ARGUMENT
    with pytest.raises(ValueError):
        t.resolve([W.TABLE[0]])
    got = K.run_single(W, W.single)
    for call in got:
        assert got[call]["stats"] == [0, 0]
        assert {k: v for k, v in got[call].items() if k != "stats"} == {k: v for k, v in with_table[call].items() if k != "stats"}
    assert got["verify_each"]["each"] == W.exp_single
    assert K.run_multi(W, W.multi)["fast_aggregate_verify_many"] == {"each": [True] * 3, "stats": [0, 0]}
    assert t.lookup_stats() == (0, 0)
    # a table of other keys: the index holds nothing of the first table
    t2 = _load(W, W.TABLE_OTHER)
    assert t2.resolve(W.TABLE[:3] + W.TABLE_OTHER[:2]) == [MISS, MISS, MISS, 0, 1]
    assert _check_single(W, K.run_single(W, W.single), W.TABLE_OTHER) == (77, 523)


def test_lookup_off_in_child(W):
    """TBLS_PK_LOOKUP=0: verdicts equal, the counters stay 0, no index to resolve from."""
    got = _child(["lookup_off"], TBLS_PK_LOOKUP="0")
    for call, v in got["single"].items():
        assert v["stats"] == [0, 0]
    assert got["single"]["batch_verify"]["ok"] is False
    assert got["single"]["verify_each"]["each"] == W.exp_single
    assert got["single"]["batch_verify_each"] == {"ok": False, "each": W.exp_single, "stats": [0, 0]}
    assert got["multi"]["fast_aggregate_verify_many"] == {"each": [True] * 3, "stats": [0, 0]}
    assert got["multi"]["batch_verify"] == {"ok": True, "stats": [0, 0]}
    assert got["resolve"] == "ValueError"


def test_two_library_devices(W):
    """Two library devices over the one GPU (TBLS_INIT_SHARE_DEVICES), each
    with its own copy of the table and index: the 600 sets shard 300 + 300,
    both shards resolve from their own device's index, the summed counts are
    exact and the verdicts equal the oracle.  A 300-set shard is below the 512
    sets up to which the default plan decodes keys inside k_keys_coop (no
    lookup), so this case runs the plan of TBLS_COOP=0, whose key stage is the
    decompress branch at every size; 1,200 sets (the same keys twice) shard
    600 + 600 under the default plan."""
    got = _child(["two_devices", "600"], TBLS_SHARD_MIN="300", TBLS_COOP="0")
    assert got["devices"] == 2 and got["batch_verify"]["n_devices"] == 2 and got["batch_verify_each"]["n_devices"] == 2
    assert _check_single(W, got, W.TABLE) == (523, 77)
    batch = W.single_times(2)
    exp = C.verify_each([[p] for p in batch[0]], batch[1], batch[2], threads=THREADS)
    assert [p for p, v in enumerate(exp) if not v] == [K.P_INF, K.P_BAD, K.P_TAMPER, 600 + K.P_INF, 600 + K.P_BAD]
    got = _child(["two_devices", "1200"], TBLS_SHARD_MIN="600")
    assert got["devices"] == 2 and got["batch_verify"]["n_devices"] == 2 and got["batch_verify_each"]["n_devices"] == 2
    assert _check_single(W, got, W.TABLE, batch=batch, exp=exp) == (1046, 154)


def test_dev_batch_partial_unaligned_keys(W):
    """tbls_dev_batch_partial with the key bytes at offset 4 (and 1) into a
    device buffer: the lookup falls back to narrower loads, and the partial
    record and its verdict equal the aligned call's."""
    import torch

    native = W.native
    L = native.lib()
    t = _load(W, W.TABLE)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pk, ms, sg = W.single_valid
    n = K.N_SINGLE
    u8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    rr = K.rands(W, n)
    bufs = dict(msgs=u8(b"".join(ms)), sigs=u8(b"".join(sg)), pk_off=torch.arange(0, n + 1, dtype=torch.int32, device=dev),
                msg_off=torch.arange(0, 32 * (n + 1), 32, dtype=torch.int32, device=dev),
                rand=torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in rr], dtype=torch.int64, device=dev))

    def partial(offset):
        keys = u8(bytes(offset) + b"".join(pk))
        assert keys.data_ptr() % 16 == 0
        d = native.TblsDevBatch(keys.data_ptr() + offset, bufs["pk_off"].data_ptr(), n, bufs["msgs"].data_ptr(), bufs["msg_off"].data_ptr(),
                                bufs["sigs"].data_ptr(), bufs["rand"].data_ptr(), n)
        out = torch.zeros(native.PARTIAL_BYTES, dtype=torch.uint8, device=dev)
        native.check(L.tbls_dev_batch_partial(0, ctypes.byref(d), stream, out.data_ptr()), "partial")
        ok = ctypes.c_int(7)
        native.check(L.tbls_dev_final_verify(0, out.data_ptr(), 1, stream, ctypes.byref(ok)), "final")
        torch.cuda.synchronize()
        return bytes(out.cpu().numpy()), ok.value

    t.lookup_stats(reset=True)
    rec0, ok0 = partial(0)
    assert ok0 == 1 and t.lookup_stats(reset=True) == (523, 77)
    for off in (4, 1):
        rec, ok = partial(off)
        assert ok == ok0 and rec == rec0
        assert t.lookup_stats(reset=True) == (523, 77)
    t.clear()
    rec, ok = partial(4)  # and the same record without a table
    assert ok == 1 and rec == rec0 and t.lookup_stats() == (0, 0)
