"""Grouped batches without a device: the four C entries are exported and
bound, tbls_group_plan answers as tb_plan.h states, and the service's
group_messages option drives the grouped entry (stub device functions with the
C oracle behind them, as tests/test_service.py)."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from oracle import c_oracle as C
from oracle.keys import interop_sk
from teku_amd import native
from teku_amd.service import AggregatingSignatureVerificationService, SignatureTask, _set_tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED_ENTRIES = ["tbls_batch_verify_grouped", "tbls_batch_verify_idx_grouped", "tbls_dev_batch_partial_grouped", "tbls_group_plan"]


def test_the_four_entries_are_exported_and_declared():
    L = ctypes.CDLL(native.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tekubls.h")).read()
    for name in GROUPED_ENTRIES:
        assert getattr(L, name) is not None
        assert name in native._SIGS and getattr(native.load_library(), name).argtypes is not None
        # each entry's comment cites the reference lines it mirrors
        decl = header.index("int " + name + "(")
        comment = header[header.rindex("/*", 0, decl):decl]
        assert "BLS.java:275-336" in comment and "AggregatingSignatureVerificationService.java" in comment and "187-227" in comment, name
    assert "TBLS_GROUP_FORCE = 1u" in header and native.GROUP_FORCE == 1


def test_group_plan_default_thresholds():
    """the built-in thresholds: a repeated message groups at least under
    TBLS_GROUP_FORCE (1 or 2), with n_msgs + 64 pairs; every message distinct
    never groups and keeps the ungrouped pairs"""
    for n, m in [(828, 8), (4096, 2048), (256, 1), (2, 1), (131072, 64)]:
        grouped, pairs = native.group_plan(n, m)
        assert grouped in (1, 2) and pairs == m + 64, (n, m)
    assert native.group_plan(4096, 2048)[1] == 2112
    for n, m in [(128, 128), (128, 0), (128, 129), (1, 1), (0, 0)]:
        grouped, pairs = native.group_plan(n, m)
        assert grouped == 0, (n, m)
        assert pairs == (2 * n if n < 20480 else n + 64), (n, m)


def test_group_plan_reads_the_environment():
    """TBLS_GROUP_MIN="min[,percent]" (read once per process: a child each)"""
    code = ("import sys; sys.path.insert(0, %r); from teku_amd import native; "
            "print([native.group_plan(n, m)[0] for n, m in [(999, 10), (1000, 10), (1000, 250), (1000, 251), (1000, 1000)]])" % ROOT)
    for env, want in [("1000,25", [1, 2, 2, 1, 0]), ("0,100", [2, 2, 2, 2, 0]), ("1000", None)]:
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TBLS_GROUP_MIN=env), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        got = eval(out.stdout.strip().splitlines()[-1])
        if want is None:  # the minimum alone keeps the built-in percent, whatever it is
            assert got[0] == 1 and got[1] == 2 and got[4] == 0
        else:
            assert got == want, env


def test_java_service_has_the_opt_in_flag():
    """the Java half: the native method, its JNI definition on
    tbls_batch_verify_grouped, and the service's groupMessages flag (default
    false) handed to the one batchVerifyEach call"""
    import re

    J = os.path.join(ROOT, "integration", "java", "tech", "pegasys", "teku")
    natives = open(os.path.join(J, "bls", "impl", "hip", "TekuBlsHipGrouped.java")).read()
    assert set(re.findall(r"static native \w+ (\w+)\(", natives)) == {"batchVerifyGrouped"}
    glue_path = os.path.join(ROOT, "integration", "native", "tekubls_grouped_jni.c")
    glue = open(glue_path).read()
    assert set(re.findall(r"JNICALL JNAME\((\w+)\)", glue)) == {"batchVerifyGrouped"}
    assert "Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipGrouped_##n" in glue
    assert set(re.findall(r"\b(tbls_\w+)\(", glue)) == {"tbls_batch_verify_grouped"}
    ver =open(os.path.join(J, "bls", "impl", "hip", "HipBatchVerifier.java")).read()
    assert "TekuBlsHipGrouped.batchVerifyGrouped(" in ver and "return batchVerifyEach(keys, messages, signatures, nGpus, okPerSet, false);" in ver
    svc = open(os.path.join(J, "statetransition", "validation", "signatures", "HipAggregatingSignatureVerificationService.java")).read()
    assert "final boolean groupMessages" in svc and "queueCapacity, maxBatchSize, false);" in svc
    assert "nGpus, okPerSet, groupMessages);" in svc
    assert "groupMessages" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_grouped_jni_glue_validates_arguments(tmp_path):
    """the glue against a stub JNI environment and a recording fake of the C
    entry (tests/native/grouped_jni_glue_test.c), a stand-alone program under
    ASan/UBSan; no JDK is needed"""
    exe = str(tmp_path / "grouped_jni_glue_test")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "native", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "integration", "native", "tekubls_grouped_jni.c"),
                           os.path.join(ROOT, "tests", "native", "grouped_jni_glue_test.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


# ---- the service -----------------------------------------------------------
@pytest.fixture(scope="module")
def gossip():
    """12 one-key tasks over 3 messages (4 signers each), as one slot's attestations"""
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
    calls = {"grouped": 0, "each": 0}

    def grouped(sets, n_gpus, timing):
        calls["grouped"] += 1
        return _oracle_batch(sets)

    def each(sets, n_gpus, timing):
        calls["each"] += 1
        v = [_oracle_batch([s]) for s in sets]
        return all(v), v

    return AggregatingSignatureVerificationService(num_threads=1, batch_each_fn=each, batch_grouped_fn=grouped, **kw), calls


def _tasks(gossip, bad=()):
    pks, msgs, sigs = gossip
    return [SignatureTask([_set_tuple([pks[i]], msgs[i], sigs[(i + 1) % 12] if i in bad else sigs[i])]) for i in range(12)]


def test_service_passing_batch_makes_one_grouped_call(gossip):
    svc, calls = _svc(group_messages=True)
    ts = _tasks(gossip)
    svc.batch_verify_signatures(ts)
    assert [t.result.result(timeout=5) for t in ts] == [True] * 12
    assert calls == {"grouped": 1, "each": 0}
    m = svc.metrics()
    assert m["grouped_batches_total"] == 1 and m["grouped_sets_per_message"] == 4.0 and m["device_passes_total"] == 1


def test_service_failing_batch_then_makes_one_each_call(gossip):
    bad = {3, 8}
    svc, calls = _svc(group_messages=True)
    ts = _tasks(gossip, bad)
    svc.batch_verify_signatures(ts)
    with_flag = [t.result.result(timeout=5) for t in ts]
    assert calls == {"grouped": 1, "each": 1}
    assert svc.metrics()["device_passes_total"] == 2 and svc.last_batch_timing["settled"] is True
    # verdicts and futures as without the flag
    ref, ref_calls = _svc()
    rs = _tasks(gossip, bad)
    ref.batch_verify_signatures(rs)
    assert ref_calls == {"grouped": 0, "each": 1}
    assert with_flag == [t.result.result(timeout=5) for t in rs] == [i not in bad for i in range(12)]
    assert all(t.result.done() and t.result.exception() is None for t in ts)
    assert ref.metrics()["grouped_batches_total"] == 0 and ref.metrics()["grouped_sets_per_message"] is None


def test_service_multi_set_tasks_and_threads(gossip):
    pks, msgs, sigs = gossip
    svc, calls = _svc(group_messages=True, max_batch_size=64)
    svc.start()
    try:
        good = svc.verify_many([[pks[0]], [pks[3]]], [msgs[0], msgs[3]], [sigs[0], sigs[3]])
        mixed = svc.verify_many([[pks[1]], [pks[4]]], [msgs[1], msgs[4]], [sigs[1], sigs[1]])
        empty = svc.verify_many([], [], [])
        assert good.result(timeout=60) is True and mixed.result(timeout=60) is False and empty.result(timeout=60) is False
    finally:
        svc.stop()
    assert calls["grouped"] >= 1
