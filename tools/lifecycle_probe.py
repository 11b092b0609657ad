"""The library's life cycle in one fresh process: tbls_init over two shared
library devices, a key table, a batch; tbls_shutdown (every context's buffers,
streams and events destroyed); tbls_init again over one device -- no table
survives -- the same batch, a tampered one; tbls_shutdown.  Prints one JSON line.

    python tools/lifecycle_probe.py

Run by tests/test_gpu_lifecycle.py as a child process, so the test session's
own library state is never shut down.
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch  # noqa: F401  (one HIP runtime: torch's, teku_amd/native.py)

    from oracle import bls12_381 as O
    from oracle.keys import interop_sk
    from teku_amd import bls, native

    sks = [interop_sk(i) for i in range(8)]
    pks = [O.sk_to_pk(s) for s in sks]
    msgs = [bytes([i]) * 32 for i in range(4)]
    sets = [(pks[i], 1, msgs[i], O.sign(sks[i], msgs[i])) for i in range(4)]
    bad = list(sets)
    bad[2] = (sets[2][0], 1, msgs[3], sets[2][3])
    rands = [3, 5, 7, 11]

    L = native.load_library()
    out = {}
    native.check(L.tbls_init(2, 1), "tbls_init(2, share devices)")
    native._lib = L  # bls.batch_verify_raw goes through native.lib()
    out["devices_first"] = L.tbls_device_count()
    native.check(L.tbls_pk_table_load(b"".join(pks), 8, None), "tbls_pk_table_load")
    out["table_first"] = L.tbls_pk_table_size()
    out["valid_first"] = bls.batch_verify_raw(sets, rands)
    L.tbls_shutdown()
    out["devices_after_shutdown"] = L.tbls_device_count()
    native.check(L.tbls_init(1, 0), "tbls_init(1) after shutdown")
    out["devices_second"] = L.tbls_device_count()
    out["table_second"] = L.tbls_pk_table_size()
    out["valid_second"] = bls.batch_verify_raw(sets, rands)
    out["tampered_second"] = bls.batch_verify_raw(bad, rands)
    L.tbls_shutdown()
    out["devices_end"] = L.tbls_device_count()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
