"""The learned key cache's index functions on the CPU
(teku_amd/csrc/tb_pkindex.h: pkx_cache, pkx_reserve, pkx_append, pkx_find_two
-- the functions k_pk_learn and k_pk_lookup run on the device): host build of
tests/native/pkcache_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer, run directly, at 8 rows / 16 slots, with the
header's probe bound and with a bound below the row count; and the two public
entries of the cache exported by the built library and bound in
teku_amd/native.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bound", [None, 3])
def test_pkcache_check(tmp_path, bound):
    exe = str(tmp_path / "pkcache_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pkcache_check.cpp"),
           "-o", exe]
    if bound is not None:
        cmd.insert(1, f"-DTB_PKX_PROBE_MAX={bound}u")
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "failures 0" in out.stdout and "FAIL" not in out.stdout, out.stdout[-4000:]


def test_cache_symbols_exported_and_bound():
    from teku_amd import bls, native

    if not os.path.exists(native.LIB_PATH):  # normally built by __graft_entry__.build()
        import __graft_entry__ as ge

        ge.build_hip_lib()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in ("tbls_pk_cache_stats", "tbls_pk_cache_clear"):
        assert hasattr(lib, s), s
        assert s in native.EXPORTED
    L = native.load_library()
    assert L.tbls_pk_cache_stats.restype is ctypes.c_int and len(L.tbls_pk_cache_stats.argtypes) == 2
    assert L.tbls_pk_cache_clear.argtypes == []
    assert callable(bls.pk_cache_stats) and callable(bls.pk_cache_clear)


def test_no_device_no_cache():
    """Without a device (or before tbls_init) the new entries fail loudly, as every entry does."""
    from teku_amd import native

    L = native.load_library()
    if L.tbls_device_count() == 0:
        out = (ctypes.c_uint64 * 4)()
        assert L.tbls_pk_cache_clear() == native.DEVICE_ERROR
        assert L.tbls_pk_cache_stats(out, 0) == native.DEVICE_ERROR
