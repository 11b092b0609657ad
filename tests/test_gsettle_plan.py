"""The scratch layout of settling a failed grouped batch on the CPU
(teku_amd/csrc/tb_plan.h gsettle_layout, TBLS_GSETTLE_CHUNK) and the verdicts'
position-to-set map over tb_group.h's CSR: tests/native/gsettle_plan_check.cpp,
a stand-alone program with its own main, built under AddressSanitizer +
UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-I", os.path.join(ROOT, "teku_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def test_gsettle_layout_and_position_map(tmp_path):
    """one line per failed check; `ok <count>` when none failed.  13 sizes x up
    to 4 message counts x 2 chunk sizes, a few dozen checks each"""
    exe = str(tmp_path / "gsettle_plan_check")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "native", "gsettle_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("ok "), out.stdout[-4000:]
    assert int(last.split()[1]) > 5000
