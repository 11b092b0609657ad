"""The per-key fixed-base comb on the CPU (teku_amd/csrc/tb_pkcomb.h:
comb_build, comb_mul_u64, the reference word and the ready bytes -- the
functions k_pk_learn_comb, k_pk_comb_build and k_set_pk_comb_w2 run on the
device): host build of tests/native/pkcomb_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer, run directly on a handful of interop keys; and the
counter entry exported by the built library and bound in teku_amd/native.py."""
import ctypes
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pkcomb_check(tmp_path):
    from oracle import bls12_381 as O
    from oracle.keys import interop_sk

    exe = str(tmp_path / "pkcomb_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pkcomb_check.cpp"),
           "-o", exe]
    subprocess.check_call(cmd)
    keys = [O.sk_to_pk(interop_sk(i)).hex() for i in range(4)]
    out = subprocess.run([exe] + keys, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "failures 0" in out.stdout and "FAIL" not in out.stdout, out.stdout[-4000:]
    assert "keys 4 " in out.stdout, out.stdout[-4000:]  # the interop keys were the ones checked


def test_comb_symbol_exported_and_bound():
    from teku_amd import bls, native

    if not os.path.exists(native.LIB_PATH):  # normally built by __graft_entry__.build()
        import __graft_entry__ as ge

        ge.build_hip_lib()
    lib = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(lib, "tbls_pk_comb_stats") and "tbls_pk_comb_stats" in native.EXPORTED
    for k in ("k_set_pk_comb_w2", "k_pk_lookup_ref", "k_pk_learn_comb", "k_pk_comb_build", "k_set_pk_w2", "k_pk_lookup", "k_pk_learn"):
        assert hasattr(lib, k), k  # the new kernels beside the ones they stand in for
    L = native.load_library()
    assert L.tbls_pk_comb_stats.restype is ctypes.c_int and len(L.tbls_pk_comb_stats.argtypes) == 2
    assert callable(bls.pk_comb_stats)
    if L.tbls_device_count() == 0:  # without a device the entry fails loudly, as every entry does
        assert L.tbls_pk_comb_stats((ctypes.c_uint64 * 4)(), 0) == native.DEVICE_ERROR


def test_mul_counts_has_the_comb_path():
    """tools/mul_counts.json: the comb path's products per set beside the window
    path's, which keeps its value (bench.py reads the file)."""
    with open(os.path.join(ROOT, "tools", "mul_counts.json")) as f:
        m = json.load(f)
    assert m["set_pk"] == 748.0
    assert 0 < m["set_pk_comb"] < 0.45 * m["set_pk"]
