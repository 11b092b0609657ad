"""Every host-side plan of the KZG batch verification, through every entry
point: the lane-cooperative or the one-lane point and term kernels
(TKZG_COOP_MAX) and the host or the device challenge hash
(TKZG_HOST_CHALLENGE_MAX), through tkzg_verify_blob_kzg_proof_batch,
tkzg_dev_verify_blob_kzg_proof_batch and its _profiled twin (another launch
order).  Both limits are read once per process, so tools/kzg_record.py runs
once per plan, one process after the other, and prints the records of a fixed
case list (tests/kzg_cases.py form_cases: n = 1, 2, 3, 5; valid, wrong proofs,
an order-11 commitment, a non-canonical element).  The records must be the same
under every plan and entry point and equal the C oracle's verdicts, challenges
z, evaluations y and batch challenge r; errors are C_KZG_BADARGS naming the
kind and the lowest offending index."""

import json
import os
import subprocess
import sys

import pytest

from oracle import kzg_oracle as K
from tests import kzg_cases as C
from tests.kzg_util import SETUP, sample_blob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANS = [{}, {"TKZG_COOP_MAX": "0"}, {"TKZG_HOST_CHALLENGE_MAX": "0"}, {"TKZG_COOP_MAX": "0", "TKZG_HOST_CHALLENGE_MAX": "0"}]
ENTRIES = ("host", "dev", "profiled")


@pytest.fixture(scope="module")
def records():
    """One child per plan, one at a time; a failed child stops the rest."""
    out = []
    for plan in PLANS:
        env = {k: v for k, v in os.environ.items() if k not in ("TKZG_COOP_MAX", "TKZG_HOST_CHALLENGE_MAX")}
        env.update(plan)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kzg_record.py")], env=env, capture_output=True, text=True, timeout=240,
                           cwd=ROOT)
        assert r.returncode == 0, (plan, r.stderr[-2000:])
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(plan, out[-1]["seconds"])
    return out


@pytest.fixture(scope="module")
def expected(records):
    """(name, kind, oracle result) per case, from the first child's commitments and proofs."""
    cs = [bytes.fromhex(x) for x in records[0]["commitments"]]
    ps = [bytes.fromhex(x) for x in records[0]["proofs"]]
    blobs = [sample_blob(s) for s in C.FORM_SEEDS]
    orc = K.Setup.from_file(SETUP)
    out = [(name, kind, orc.verify_blob_kzg_proof_batch(b, c, p, detail=True)) for name, kind, b, c, p in C.form_cases(blobs, cs[:5], ps[:5], ps[5])]
    orc.close()
    return out


def test_same_records_under_every_plan_and_entry(records):
    first = records[0]
    for plan, rec in zip(PLANS, records):
        assert rec["commitments"] == first["commitments"] and rec["proofs"] == first["proofs"], plan
        assert [c["case"] for c in rec["cases"]] == [c["case"] for c in first["cases"]]
        for c, c0 in zip(rec["cases"], first["cases"]):
            for e in ENTRIES:
                assert c[e] == c0["host"], (plan, c["case"], e)


def test_records_match_oracle(records, expected):
    cases = records[0]["cases"]
    assert [c["case"] for c in cases] == [name for name, _, _ in expected]
    for c, (name, kind, (res, zs, ys, r)) in zip(cases, expected):
        got = c["host"]
        if kind in ("valid", "false"):
            assert res is (kind == "valid"), name  # the oracle's own verdict
            assert got["rc"] == 0 and got["ok"] is res, (name, got)
            assert got["zs"] == [z.hex() for z in zs] and got["ys"] == [y.hex() for y in ys] and got["r"] == r.hex(), name
        else:
            assert res == K.KZG_BADARGS, name
            assert got == {"rc": 1, "msg": kind}, (name, got)


def test_misaligned_device_pointer_is_badargs(records):
    for plan, rec in zip(PLANS, records):
        assert rec["misaligned"]["rc"] == 1 and "16-byte aligned" in rec["misaligned"]["msg"], (plan, rec["misaligned"])
