"""The JNI glue of the grouped batch-and-settle entry (integration/native/
tekubls_grouped_each_jni.c) and the Java half's opt-in flag, without a JDK or a
device: the glue runs against a stub JNI environment and a recording fake of
tbls_batch_verify_each_grouped (tests/native/grouped_each_jni_glue_test.c), a
stand-alone program under ASan/UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = os.path.join(ROOT, "integration", "java", "tech", "pegasys", "teku")


def test_glue_validates_arguments_and_returns_both_verdicts(tmp_path):
    exe = str(tmp_path / "grouped_each_jni_glue_test")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "native", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "integration", "native", "tekubls_grouped_each_jni.c"),
                           os.path.join(ROOT, "tests", "native", "grouped_each_jni_glue_test.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_java_half_has_the_opt_in_flag():
    """the native method and its JNI definition on tbls_batch_verify_each_grouped
    alone; HipBatchVerifier.batchVerifyEachGrouped; the service's groupSettle
    flag, false from every existing constructor"""
    natives = open(os.path.join(J, "bls", "impl", "hip", "TekuBlsHipGroupedEach.java")).read()
    assert set(re.findall(r"static native \w+ (\w+)\(", natives)) == {"batchVerifyEachGrouped"}
    glue = open(os.path.join(ROOT, "integration", "native", "tekubls_grouped_each_jni.c")).read()
    assert set(re.findall(r"JNICALL JNAME\((\w+)\)", glue)) == {"batchVerifyEachGrouped"}
    assert "Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipGroupedEach_##n" in glue
    assert set(re.findall(r"\b(tbls_\w+)\(", glue)) == {"tbls_batch_verify_each_grouped"}
    ver = open(os.path.join(J, "bls", "impl", "hip", "HipBatchVerifier.java")).read()
    assert "TekuBlsHipGroupedEach.batchVerifyEachGrouped(" in ver and "boolean groupSettle" in ver
    assert "return batchVerifyEach(keys, messages, signatures, nGpus, okPerSet, groupMessages, false);" in ver
    svc = open(os.path.join(J, "statetransition", "validation", "signatures", "HipAggregatingSignatureVerificationService.java")).read()
    assert "final boolean groupSettle" in svc and "groupMessages && groupSettle" in svc
    assert svc.count("HipBatchVerifier.batchVerifyEachGrouped(") == 1 and "public static boolean batchVerifyEachGrouped(" in ver
    assert svc.count("maxBatchSize, groupMessages,\n        false);") == 1  # the six-argument constructor keeps today's path
    assert "groupSettle" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
