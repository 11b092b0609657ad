"""Consistency of the sync-committee Java/JNI sources with the C ABI, as
tests/test_integration_sources.py checks the existing pair: every `native`
method of TekuBlsHipCommittee has its JNI definition in
integration/native/tekubls_committee_jni.c and vice versa, and the glue calls
only functions include/tekubls.h declares."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = os.path.join(ROOT, "integration", "java", "tech", "pegasys", "teku", "bls", "impl", "hip")
N = os.path.join(ROOT, "integration", "native")


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def _natives(java):
    return set(re.findall(r"static native \w+(?:\[\])? (\w+)\(", java))


def test_committee_natives_match_glue():
    java = _read(J, "TekuBlsHipCommittee.java")
    c = _read(N, "tekubls_committee_jni.c")
    jni = set(re.findall(r"JNICALL JNAME\((\w+)\)", c))
    assert _natives(java) == jni == {"fastAggregateVerifyManyIdx", "committeeLoad", "fastAggregateVerifyManyBits"}
    assert "Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipCommittee_##n" in c
    declared = set(re.findall(r"\b(tbls_\w+)\(", _read(ROOT, "include", "tekubls.h")))
    called = set(re.findall(r"\b(tbls_\w+)\(", c))
    assert called <= declared
    assert {"tbls_fast_aggregate_verify_many_idx", "tbls_committee_load", "tbls_fast_aggregate_verify_many_bits"} <= called


def test_committee_natives_not_in_existing_pair():
    """The existing class and glue stay as they were (their own tests pin
    them to each other and to a fixed fake of the C ABI)."""
    assert not _natives(_read(J, "TekuBlsHip.java")) & _natives(_read(J, "TekuBlsHipCommittee.java"))
    assert "committee" not in _read(N, "tekubls_jni.c").lower()


def test_verifier_reaches_the_committee_natives():
    ver = _read(J, "HipBatchVerifier.java")
    assert "public static boolean[] fastAggregateVerifyCommittee(" in ver and "TekuBlsHipCommittee.fastAggregateVerifyManyBits(" in ver
    assert "public static void loadCommittee(" in ver and "TekuBlsHipCommittee.committeeLoad(" in ver
