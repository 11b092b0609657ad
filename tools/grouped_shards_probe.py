"""Grouped batches over two shards on one GPU: a fresh process initialises the
library with TBLS_INIT_SHARE_DEVICES (2 library devices over the visible
hardware) and, with TBLS_SHARD_MIN=256 in the environment, a lone batch of 512
sets is cut in two.  The sets sign 4 messages in turn (set i signs message
i mod 4), so every group straddles the cut and each shard groups its own 256
sets into 4 groups of 64 (tb_lib.hip shard_launch).  The batch runs through
tbls_batch_verify_grouped with TBLS_GROUP_FORCE, valid and with one signature
replaced in the second shard; the C oracle checks the same sets with the same
randomizers.  Prints one JSON line.

    TBLS_SHARD_MIN=256 python tools/grouped_shards_probe.py

Run by tests/test_gpu_grouped.py as a child process.
"""

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
    n, m = 512, 4
    sks = [synth.interop_sk(i) for i in range(n)]
    pk = synth.pubkeys(sks)
    roots = [synth.bench_message(33, g) for g in range(m)]
    ms = [roots[i % m] for i in range(n)]
    blob = synth.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    rands = synth.random_multipliers(n)
    out = {"devices": L.tbls_device_count(), "shard_min": L.tbls_shard_min(), "group_plan": list(native.group_plan(n // 2, m)), "cases": []}
    for name, j in (("valid", None), ("one bad signature", 300)):
        s = list(sg)
        if j is not None:
            s[j] = sg[j + 1]  # another key's signature on another message
        arr = synth.SetArray(b"".join(pk), [1] * n, b"".join(ms), [len(x) for x in ms], b"".join(s))
        t = native.TblsTiming()
        native.stats(reset=True)
        got = arr.batch_verify_grouped(rands, force=True, timing=t)
        st = native.stats()
        out["cases"].append({"name": name, "got": got, "plain": arr.batch_verify(rands), "oracle": C.batch_verify(pk, ms, s, rands, threads=16),
                             "n_devices": t.n_devices, "partials": st["partials"]})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
