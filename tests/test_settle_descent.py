"""The group-test descent of settling a failed batch on the CPU
(teku_amd/csrc/tb_settle.h settle_descent, which tb_lib.hip settle_tail runs
over the device's group tests): tests/native/settle_descent_check.cpp, a
stand-alone program with its own main that drives the descent with a simulated
tester, built under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-I", os.path.join(ROOT, "teku_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def test_settle_descent(tmp_path):
    """one line per failed check; `ok <count>` when none failed.  8 sizes x 3
    code arrays x 8 patterns of invalid sets, at least 8 checks each"""
    exe = str(tmp_path / "settle_descent_check")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "native", "settle_descent_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("ok "), out.stdout[-4000:]
    assert int(last.split()[1]) >= 8 * 3 * 8 * 8
