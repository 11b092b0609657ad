"""The key table's index over its compressed key bytes on the CPU
(teku_amd/csrc/tb_pkindex.h: hash, probe step, probe bound, insertion, lookup
-- the functions the device runs): host build of tests/native/pkindex_check.cpp
under AddressSanitizer + UndefinedBehaviorSanitizer, run directly, with the
header's probe bound and with a bound below the capacity; and the three
public entries of the index exported by the built library and bound in
teku_amd/native.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bound", [None, 3])
def test_pkindex_check(tmp_path, bound):
    exe = str(tmp_path / "pkindex_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pkindex_check.cpp"), "-o", exe]
    if bound is not None:
        cmd.insert(1, f"-DTB_PKX_PROBE_MAX={bound}u")
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "failures 0" in out.stdout and "FAIL" not in out.stdout, out.stdout[-4000:]


def test_header_names_the_probe_bound():
    src = open(os.path.join(ROOT, "teku_amd", "csrc", "tb_pkindex.h")).read()
    assert "#define TB_PKX_PROBE_MAX 64u" in src


NEW = ("tbls_pk_table_resolve", "tbls_pk_lookup_stats", "tbls_pk_table_clear")


def test_new_symbols_exported_and_bound():
    from teku_amd import native

    if not os.path.exists(native.LIB_PATH):  # normally built by __graft_entry__.build()
        import __graft_entry__ as ge

        ge.build_hip_lib()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in native.EXPORTED
    L = native.load_library()
    assert L.tbls_pk_table_resolve.restype is ctypes.c_int and len(L.tbls_pk_table_resolve.argtypes) == 3
    assert len(L.tbls_pk_lookup_stats.argtypes) == 2 and L.tbls_pk_table_clear.argtypes == []
    from teku_amd import bls

    for m in ("resolve", "lookup_stats", "clear"):
        assert callable(getattr(bls.ValidatorKeyTable, m))


def test_no_device_no_table():
    """Without a device (or before tbls_init) the new entries fail loudly, as every entry does."""
    from teku_amd import native

    L = native.load_library()
    if L.tbls_device_count() == 0:
        out = (ctypes.c_uint64 * 2)()
        idx = (ctypes.c_uint32 * 1)()
        assert L.tbls_pk_table_clear() == native.DEVICE_ERROR
        assert L.tbls_pk_lookup_stats(out, 0) == native.DEVICE_ERROR
        assert L.tbls_pk_table_resolve(bytes(48), 1, idx) == native.DEVICE_ERROR
