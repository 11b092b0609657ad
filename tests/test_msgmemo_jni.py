"""The hash-point memo's Java/JNI sources (TekuBlsHipMemo.java,
integration/native/tekubls_memo_jni.c) and its C ABI: every `native` method
has its JNI definition and vice versa, the glue calls only functions
include/tekubls.h declares, the services carry their option; the glue compiled
with gcc against the stub JNI environment (tests/native/jni_stub/jni.h) and a
recording fake of the entries it calls, under ASan/UBSan, run as a plain
executable (tests/native/memo_jni_glue_test.c; no JDK is needed); and the three
entries exported by the built library, declared in the header with their
reference citations and bound in teku_amd/native.py."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = os.path.join(ROOT, "integration", "java", "tech", "pegasys", "teku")
N = os.path.join(ROOT, "integration", "native")
ENTRIES = ("tbls_msg_memo_configure", "tbls_msg_memo_stats", "tbls_msg_memo_clear")


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def test_memo_natives_match_glue():
    java = _read(J, "bls", "impl", "hip", "TekuBlsHipMemo.java")
    c = _read(N, "tekubls_memo_jni.c")
    natives = set(re.findall(r"static native \w+(?:\[\])? (\w+)\(", java))
    jni = set(re.findall(r"JNICALL JNAME\((\w+)\)", c))
    assert natives == jni == {"msgMemoConfigure", "msgMemoStats", "msgMemoClear"}
    assert "Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipMemo_##n" in c
    declared = set(re.findall(r"\b(tbls_\w+)\(", _read(ROOT, "include", "tekubls.h")))
    called = set(re.findall(r"\b(tbls_\w+)\(", c))
    assert called <= declared and set(ENTRIES) <= called


def test_services_carry_the_option():
    svc = _read(J, "statetransition", "validation", "signatures", "HipAggregatingSignatureVerificationService.java")
    ver = _read(J, "bls", "impl", "hip", "HipBatchVerifier.java")
    assert "final int hashMemoRows" in svc and "HipBatchVerifier.configureHashMemo(hashMemoRows)" in svc
    assert "public static void configureHashMemo(" in ver and "TekuBlsHipMemo.msgMemoConfigure(" in ver
    py = _read(ROOT, "teku_amd", "service.py")
    assert "hash_memo_rows: int = 0" in py and "msg_memo_configure(self.hash_memo_rows)" in py


def test_header_cites_the_reference():
    h = _read(ROOT, "include", "tekubls.h")
    block = h[h.index("---- hash-point memo ----"):]
    block = block[: block.index("int tbls_msg_memo_clear(void);")]
    assert "AggregatingSignatureVerificationService.java:187-227" in block and "HashToCurve.java:24-31" in block
    for e in ENTRIES:
        assert re.search(r"^int %s\(" % e, h, re.M), e


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_memo_jni_glue_validates_arguments(tmp_path):
    exe = str(tmp_path / "memo_jni_glue_test")
    cmd = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "native", "jni_stub"), "-I", os.path.join(ROOT, "include"),
           os.path.join(N, "tekubls_memo_jni.c"), os.path.join(ROOT, "tests", "native", "memo_jni_glue_test.c"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_memo_symbols_exported_and_bound():
    from teku_amd import bls, native

    if not os.path.exists(native.LIB_PATH):  # normally built by __graft_entry__.build()
        import __graft_entry__ as ge

        ge.build_hip_lib()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in ENTRIES:
        assert hasattr(lib, s), s
        assert s in native.EXPORTED
    L = native.load_library()
    assert L.tbls_msg_memo_configure.restype is ctypes.c_int and L.tbls_msg_memo_configure.argtypes == [ctypes.c_uint32]
    assert L.tbls_msg_memo_stats.restype is ctypes.c_int and len(L.tbls_msg_memo_stats.argtypes) == 2
    assert L.tbls_msg_memo_clear.restype is ctypes.c_int and L.tbls_msg_memo_clear.argtypes == []
    assert callable(bls.msg_memo_configure) and callable(bls.msg_memo_stats) and callable(bls.msg_memo_clear)
    with pytest.raises(ValueError):
        bls.msg_memo_configure(-1)


def test_no_device_no_memo():
    """Without a device (or before tbls_init) the new entries fail loudly, as every entry does."""
    from teku_amd import native

    L = native.load_library()
    if L.tbls_device_count() == 0:
        out = (ctypes.c_uint64 * 4)()
        assert L.tbls_msg_memo_configure(4) == native.DEVICE_ERROR
        assert L.tbls_msg_memo_stats(out, 0) == native.DEVICE_ERROR
        assert L.tbls_msg_memo_clear() == native.DEVICE_ERROR
