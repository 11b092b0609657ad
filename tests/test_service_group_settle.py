"""The service's group_settle option without a device: with group_messages and
group_settle a batch is one call of the grouped batch-and-settle entry
(batch_each_grouped_fn, tbls_batch_verify_each_grouped on the device); without
group_settle the path is the two-call one of group_messages.  Stub device
functions with the C oracle behind them, as tests/test_grouped_cpu.py."""
import random

import pytest

from oracle import c_oracle as C
from oracle.keys import interop_sk
from teku_amd import native
from teku_amd.service import AggregatingSignatureVerificationService, SignatureTask, _set_tuple


@pytest.fixture(scope="module")
def gossip():
    """12 one-key tasks over 3 messages (4 signers each)"""
    sks = [interop_sk(i) for i in range(12)]
    pks = [C.sk_to_pk(s) for s in sks]
    msgs = [bytes([i % 3 + 1]) * 32 for i in range(12)]
    sigs = [C.sign(s, m) for s, m in zip(sks, msgs)]
    return pks, msgs, sigs


def _oracle_batch(sets):
    rng = random.Random(len(sets))
    if len(sets) == 1:
        sets = sets * 2
    return C.batch_verify([s[0] for s in sets], [s[2] for s in sets], [s[3] for s in sets], [rng.getrandbits(63) | 1 for _ in sets])


def _svc(**kw):
    calls = {"grouped": 0, "each": 0, "each_grouped": 0}

    def grouped(sets, n_gpus, timing):
        calls["grouped"] += 1
        return _oracle_batch(sets)

    def each(sets, n_gpus, timing):
        calls["each"] += 1
        v = [_oracle_batch([s]) for s in sets]
        return all(v), v

    def each_grouped(sets, n_gpus, timing):
        calls["each_grouped"] += 1
        assert isinstance(timing, native.TblsTiming) and n_gpus in (0, 1)
        v = [_oracle_batch([s]) for s in sets]
        return all(v), v

    return AggregatingSignatureVerificationService(num_threads=1, batch_each_fn=each, batch_grouped_fn=grouped, batch_each_grouped_fn=each_grouped,
                                                   **kw), calls


def _tasks(gossip, bad=()):
    pks, msgs, sigs = gossip
    return [SignatureTask([_set_tuple([pks[i]], msgs[i], sigs[(i + 1) % 12] if i in bad else sigs[i])]) for i in range(12)]


def test_one_pass_per_batch(gossip):
    svc, calls = _svc(group_messages=True, group_settle=True)
    ts = _tasks(gossip)
    svc.batch_verify_signatures(ts)
    assert [t.result.result(timeout=5) for t in ts] == [True] * 12
    assert calls == {"grouped": 0, "each": 0, "each_grouped": 1}
    assert svc.metrics()["device_passes_total"] == 1 and svc.last_batch_timing["settled"] is False
    bad = {3, 8}
    ts = _tasks(gossip, bad)
    svc.batch_verify_signatures(ts)
    assert [t.result.result(timeout=5) for t in ts] == [i not in bad for i in range(12)]
    assert calls == {"grouped": 0, "each": 0, "each_grouped": 2}
    m = svc.metrics()
    assert m["device_passes_total"] == 2 and m["grouped_batches_total"] == 2 and m["grouped_sets_per_message"] == 4.0
    assert svc.last_batch_timing["settled"] is True and svc.last_batch_timing["sets"] == 12
    assert all(t.result.done() and t.result.exception() is None for t in ts)


def test_multi_set_tasks_take_all_of_their_verdicts(gossip):
    pks, msgs, sigs = gossip
    svc, calls = _svc(group_messages=True, group_settle=True)
    sets = [_set_tuple([pks[i]], msgs[i], sigs[i]) for i in range(12)]
    sets[7] = _set_tuple([pks[7]], msgs[7], sigs[8])
    tasks = [SignatureTask(sets[0:3]), SignatureTask(sets[3:6]), SignatureTask(sets[6:9]), SignatureTask(sets[9:12]), SignatureTask([])]
    svc.batch_verify_signatures(tasks)
    assert [t.result.result(timeout=5) for t in tasks] == [True, True, False, True, False]
    assert calls == {"grouped": 0, "each": 0, "each_grouped": 1} and svc.metrics()["device_passes_total"] == 1


def test_without_group_settle_the_hook_is_never_called(gossip):
    bad = {5}
    for kw in ({"group_messages": True}, {"group_messages": True, "group_settle": False}, {"group_settle": True}, {}):
        svc, calls = _svc(**kw)
        ts = _tasks(gossip, bad)
        svc.batch_verify_signatures(ts)
        assert [t.result.result(timeout=5) for t in ts] == [i not in bad for i in range(12)]
        assert calls["each_grouped"] == 0, kw
        assert calls == ({"grouped": 1, "each": 1, "each_grouped": 0} if kw.get("group_messages") else {"grouped": 0, "each": 1, "each_grouped": 0}), kw
        assert svc.metrics()["device_passes_total"] == (2 if kw.get("group_messages") else 1)


def test_the_entry_is_declared_and_bound():
    """the C entry's comment cites the reference lines it mirrors"""
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tekubls.h")).read()
    fn = native.load_library().tbls_batch_verify_each_grouped
    assert fn.argtypes is not None and len(fn.argtypes) == 8 and "tbls_batch_verify_each_grouped" in native.EXPORTED
    decl = header.index("int tbls_batch_verify_each_grouped(")
    comment = header[header.rindex("/*", 0, decl):decl]
    assert "BLS.java:185-207,275-336" in comment and "AggregatingSignatureVerificationService.java:187-233" in comment
