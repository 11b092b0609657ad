"""Print the KZG batch verification's records of a fixed seeded case list as one
JSON line: per case (tests/kzg_cases.py form_cases) and per entry point --
tkzg_verify_blob_kzg_proof_batch on host memory, tkzg_dev_verify_blob_kzg_proof_batch
and its _profiled twin on torch device buffers -- the verdict or the error
code and message and, where the call succeeded, tkzg_last_transcript's zs, ys
and r; then a device call whose blob pointer is 8 bytes off the 16-byte
alignment.  The plans follow the environment (TKZG_COOP_MAX,
TKZG_HOST_CHALLENGE_MAX: read once per process), so
tests/test_gpu_kzg_forms.py runs this once per plan and compares the records.

    python tools/kzg_record.py
"""

import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from teku_amd import kzg  # noqa: E402
from tests import kzg_cases as C  # noqa: E402
from tests.kzg_util import SETUP, sample_blob  # noqa: E402


def main():
    t0 = time.time()
    device = torch.device("cuda", 0)
    ck = kzg.CKZG4844.get_instance()
    ck.load_trusted_setup(SETUP)
    L = kzg.lib()
    blobs = [sample_blob(s) for s in C.FORM_SEEDS + (C.FORM_OTHER_SEED,)]
    cs = ck.blobs_to_kzg_commitments(blobs)
    ps = [ck.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, cs)]
    t_setup = time.time() - t0

    def record(rc, ok, n):
        if rc != kzg.C_KZG_OK:
            return {"rc": rc, "msg": L.tkzg_last_error().decode(errors="replace")}
        zs, ys, r = ck.last_transcript(n)
        return {"rc": rc, "ok": bool(ok.value), "zs": [z.hex() for z in zs], "ys": [y.hex() for y in ys], "r": r.hex()}

    def dev(x):
        return torch.frombuffer(bytearray(x), dtype=torch.uint8).to(device)

    out = []
    for name, _, b, c, p in C.form_cases(blobs[:5], cs[:5], ps[:5], ps[5]):
        n = len(b)
        fb, fc, fp = b"".join(b), b"".join(c), b"".join(p)
        rec = {"case": name}
        ok = ctypes.c_int(-1)
        rec["host"] = record(L.tkzg_verify_blob_kzg_proof_batch(ctypes.byref(ok), fb, len(fb), fc, len(fc), fp, len(fp), n), ok, n)
        db, dc, dp = dev(fb), dev(fc), dev(fp)
        torch.cuda.synchronize()
        for key, fn in (("dev", L.tkzg_dev_verify_blob_kzg_proof_batch), ("profiled", L.tkzg_dev_verify_blob_kzg_proof_batch_profiled)):
            ok = ctypes.c_int(-1)
            rec[key] = record(fn(ctypes.byref(ok), db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, None), ok, n)
        out.append(rec)
    # a blob pointer 8 bytes off: refused before anything is read (the buffer is long enough all the same)
    fb, fc, fp = blobs[0], cs[0], ps[0]
    db, dc, dp = dev(fb + bytes(16)), dev(fc), dev(fp)
    torch.cuda.synchronize()
    ok = ctypes.c_int(-1)
    rc = L.tkzg_dev_verify_blob_kzg_proof_batch(ctypes.byref(ok), db.data_ptr() + 8, dc.data_ptr(), dp.data_ptr(), 1, None)
    misaligned = {"rc": rc, "msg": L.tkzg_last_error().decode(errors="replace") if rc else ""}
    print(json.dumps({"commitments": [c.hex() for c in cs], "proofs": [p.hex() for p in ps], "cases": out, "misaligned": misaligned,
                      "seconds": {"setup_and_proofs": round(t_setup, 3), "total": round(time.time() - t0, 3)}}))


if __name__ == "__main__":
    main()
