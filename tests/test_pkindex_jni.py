"""The key-index Java/JNI sources (TekuBlsHipPkIndex.java,
integration/native/tekubls_pkindex_jni.c): every `native` method has its JNI
definition and vice versa, the glue calls only functions include/tekubls.h
declares, the existing class and glue stay as they were; and the glue compiled
with gcc against the stub JNI environment (tests/native/jni_stub/jni.h) and a
recording fake of the entries it calls, under ASan/UBSan, run as a plain
executable (tests/native/pkindex_jni_glue_test.c).  No JDK is needed."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = os.path.join(ROOT, "integration", "java", "tech", "pegasys", "teku", "bls", "impl", "hip")
N = os.path.join(ROOT, "integration", "native")


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def _natives(java):
    return set(re.findall(r"static native \w+(?:\[\])? (\w+)\(", java))


def test_pkindex_natives_match_glue():
    java = _read(J, "TekuBlsHipPkIndex.java")
    c = _read(N, "tekubls_pkindex_jni.c")
    jni = set(re.findall(r"JNICALL JNAME\((\w+)\)", c))
    assert _natives(java) == jni == {"pkTableResolve", "pkTableClear"}
    assert "Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipPkIndex_##n" in c
    declared = set(re.findall(r"\b(tbls_\w+)\(", _read(ROOT, "include", "tekubls.h")))
    called = set(re.findall(r"\b(tbls_\w+)\(", c))
    assert called <= declared
    assert {"tbls_pk_table_resolve", "tbls_pk_table_clear"} <= called


def test_pkindex_natives_not_in_existing_pairs():
    new = _natives(_read(J, "TekuBlsHipPkIndex.java"))
    assert not new & _natives(_read(J, "TekuBlsHip.java"))
    assert not new & _natives(_read(J, "TekuBlsHipCommittee.java"))
    assert "resolve" not in _read(N, "tekubls_jni.c").lower()


def test_public_key_memoizes_the_index():
    pk = _read(J, "HipPublicKey.java")
    assert "TekuBlsHipPkIndex.pkTableResolve(" in pk and "tableIndex" in pk
    doc = " ".join(_read(ROOT, "INTEGRATION.md").split())
    assert "`HipPublicKey` memoizes the table index" in doc and "tbls_pk_table_resolve" in doc


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_pkindex_jni_glue_validates_arguments(tmp_path):
    exe = str(tmp_path / "pkindex_jni_glue_test")
    cmd = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "native", "jni_stub"), "-I", os.path.join(ROOT, "include"),
           os.path.join(N, "tekubls_pkindex_jni.c"), os.path.join(ROOT, "tests", "native", "pkindex_jni_glue_test.c"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
