"""Settling a failed grouped batch over two shards and several chunks on one
GPU: a fresh process initialises the library with TBLS_INIT_SHARE_DEVICES (2
library devices over the visible hardware) and, with TBLS_SHARD_MIN=256 and
TBLS_GSETTLE_CHUNK=256 in the environment, a lone batch of 1,024 sets is cut
in two shards of 512, and a failed shard settles its 512 positions in two
chunks.  The sets sign 8 messages in turn (set i signs message i mod 8), so
every group straddles the cut.  Two cases through
tbls_batch_verify_each_grouped with TBLS_GROUP_FORCE: bad signatures at sets
255, 256 and 700 (both shards fail and settle), and at set 700 alone (only the
second shard settles).  The C oracle's per-set verdicts are the reference.
Prints one JSON line.

    TBLS_SHARD_MIN=256 TBLS_GSETTLE_CHUNK=256 python tools/grouped_each_probe.py

Run by tests/test_gpu_grouped_each.py as a child process.
"""

import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch  # noqa: F401  (one HIP runtime: torch's, teku_amd/native.py)

    from oracle import c_oracle as C
    from teku_amd import native, synth

    L = native.load_library()
    native.check(L.tbls_init(2, 1), "tbls_init(share devices)")
    native._lib = L
    n, m = 1024, 8
    sks = [synth.interop_sk(i) for i in range(n)]
    pk = synth.pubkeys(sks)
    roots = [synth.bench_message(35, g) for g in range(m)]
    ms = [roots[i % m] for i in range(n)]
    blob = synth.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    rands = synth.random_multipliers(n)
    rr = (ctypes.c_uint64 * n)(*rands)
    out = {"devices": L.tbls_device_count(), "shard_min": L.tbls_shard_min(), "group_plan": list(native.group_plan(n // 2, m)), "cases": []}
    for bad in ([255, 256, 700], [700]):
        s = list(sg)
        for j in bad:
            s[j] = sg[j + 1]  # another key's signature on another message
        exp = [True] * n
        for j, v in zip(bad, C.verify_each([[pk[j]] for j in bad], [ms[j] for j in bad], [s[j] for j in bad], threads=4)):
            exp[j] = v
        arr = synth.SetArray(b"".join(pk), [1] * n, b"".join(ms), [len(x) for x in ms], b"".join(s))
        t = native.TblsTiming()
        ok, ok_p = ctypes.c_int(-1), ctypes.c_int(-1)
        each, each_p = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        native.stats(reset=True)
        rc = L.tbls_batch_verify_each_grouped(arr.ptr, n, rr, 0, native.GROUP_FORCE, ctypes.byref(ok), each, ctypes.byref(t))
        st = native.stats()
        rc_p = L.tbls_batch_verify_each(arr.ptr, n, rr, 0, ctypes.byref(ok_p), each_p, None)
        got = [v == 1 for v in each]
        out["cases"].append({"bad": bad, "rc": rc, "rc_plain": rc_p, "ok": ok.value == 1, "failed": [i for i in range(n) if not got[i]],
                             "mismatch": [i for i in range(n) if got[i] != exp[i] or each[i] != each_p[i]] + ([] if ok.value == ok_p.value else [-1]),
                             "n_devices": t.n_devices, "partials": st["partials"], "settled": st["settled"], "each_passes": st["each_passes"]})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
