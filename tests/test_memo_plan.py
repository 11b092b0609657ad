"""The batch plan, the workspace layout and the staging image with the
hash-point memo, on the CPU: a host build of tests/native/memo_plan_check.cpp
under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.

What it checks (teku_amd/csrc/tb_plan.h, tb_msgmemo.h): with the memo off every
workspace offset and the total are what they are with the new plan parameter
left at its default, at n = 8, 600, 2,304 and 16,384; with it on, Qh / skiph
hold the messages to hash, lie behind every other region and are 16-byte
aligned; the hash kernel follows the messages to hash (16,384 sets with 3 to
hash: coop; with none: none); the w2 kernel's park area fits the line buffer
at 65,536 sets with 40,000 to hash, split plan or not; and the image's new
regions follow the old ones, whose offsets and bytes stay as they are."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memo_plan_check(tmp_path):
    exe = str(tmp_path / "memo_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "memo_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env={k: v for k, v in os.environ.items() if not k.startswith("TBLS_")})
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("ok "), out.stdout[-4000:]
    assert int(last.split()[1]) >= 100
