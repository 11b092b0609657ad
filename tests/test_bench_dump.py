"""bench.py's --dump-outputs files (host logic only): a partial record goes out
as the canonical Fp12 coordinates, whatever weakly reduced Montgomery
representative the record held.  bench.py sets the HIP runtime's queue count
for its own process when imported, so it is loaded in a child process."""

import os
import subprocess
import sys

import numpy as np

from teku_amd.dist import P_MOD, R_MONT, encode_partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_canonical_float32(tmp_path):
    coords = [(0x1234567 * (k + 1) ** 7 + k) % P_MOD for k in range(12)]
    coords[0], coords[1] = 0, P_MOD - 1
    c = [(coords[2 * i], coords[2 * i + 1]) for i in range(6)]
    rec0 = bytearray(encode_partial(((c[0], c[1], c[2]), (c[3], c[4], c[5])), 3))
    # rank 1's record: the same value with one coordinate as its other representative below 2p
    rec1 = bytearray(rec0)
    m = coords[2] * R_MONT % P_MOD + P_MOD
    assert m < 2 * P_MOD and m < 1 << 384
    rec1[96:144] = m.to_bytes(48, "little")
    (tmp_path / "records.bin").write_bytes(bytes(rec0 + rec1))
    code = ("import sys, bench; bench.dump_outputs(sys.argv[2], open(sys.argv[1], 'rb').read(), 2, 1)")
    subprocess.run([sys.executable, "-c", code, str(tmp_path / "records.bin"), str(tmp_path / "out")], check=True, cwd=ROOT, timeout=120)
    fp12 = np.load(tmp_path / "out" / "partial_fp12.npy")
    assert fp12.dtype == np.float32 and fp12.shape == (2, 12, 48)
    want = np.array([list(v.to_bytes(48, "big")) for v in coords], dtype=np.float32)
    assert np.array_equal(fp12[0], want) and np.array_equal(fp12[1], want)
    bad = np.load(tmp_path / "out" / "partial_invalid_sets.npy")
    assert bad.dtype == np.float32 and bad.tolist() == [3.0, 3.0]
    verdict = np.load(tmp_path / "out" / "verdict.npy")
    assert verdict.dtype == np.float32 and verdict.tolist() == [1.0]


def test_plain_and_full_options_exist():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "--full" in out and "--dump-outputs" in out and "--steps" in out
