"""The batch plan (teku_amd/csrc/tb_plan.h: kernel choice per stage, pair
split, product levels, workspace layout) on the CPU: host build of
tests/native/plan_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer.

The dump at every size where a decision flips equals tests/golden/batch_plan.txt,
which was printed by the planning code of tb_lib.hip before it moved into the
header (so the move changed no decision); the invariants hold under the
default settings and under the overrides the GPU tests use."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "plan_check.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TBLS_")}  # the dump is the default plan

    def run(mode):
        out = subprocess.run([exe, mode], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
        return out.stdout

    return run


def test_plan_matches_table(plan_check):
    got = plan_check("dump").splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "batch_plan.txt")).read().splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_plan_invariants(plan_check):
    out = plan_check("check")
    assert "failures 0" in out and "FAIL" not in out, out[-4000:]
