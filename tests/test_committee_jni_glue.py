"""The sync-committee JNI glue (integration/native/tekubls_committee_jni.c)
compiled with gcc against the stub JNI environment (tests/native/jni_stub/jni.h)
and its own recording fake of the C ABI entries it calls, under ASan/UBSan, and
run as a plain executable: short bit arrays, non-monotone message offsets, too
few signatures or indices and small output arrays return TBLS_BAD_ARGUMENT
without reaching the library or reading past a copied array; well-formed
arguments reach it as the Java side flattened them
(tests/native/committee_jni_glue_test.c).  No JDK is needed."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_committee_jni_glue_validates_arguments(tmp_path):
    exe = str(tmp_path / "committee_jni_glue_test")
    cmd = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "native", "jni_stub"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "integration", "native", "tekubls_committee_jni.c"),
           os.path.join(ROOT, "tests", "native", "committee_jni_glue_test.c"), "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
