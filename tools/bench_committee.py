"""Sync-committee verification (config 2 shape): 64 sets over one 512-member
committee, 507 participants per set chosen from a fixed seed, through the
three paths of the C ABI in one process on one build:

  bytes  tbls_fast_aggregate_verify_many        keys as 48-byte encodings
  idx    tbls_fast_aggregate_verify_many_idx    keys by index into the table
  bits   tbls_fast_aggregate_verify_many_bits   resident committee + bitvectors

Every path gets its arguments as prebuilt C arrays (no per-call Python
marshalling); the calls are interleaved round-robin, timed on the host clock
around the blocking call, and reported as p50 over --reps calls after
--warmup.  Writes one JSON object to --out and prints it."""

import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--participants", type=int, default=507)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--order", default="bytes,idx,bits", help="the round-robin order of the paths within an iteration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "committee_cfg2.json"))
    a = ap.parse_args()
    assert a.reps >= 50, "p50 over at least 50 calls"
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import bls, native, synth

    L = native.lib()
    n, size = a.sets, a.size
    sks = [synth.interop_sk(i) for i in range(size)]
    pks = synth.pubkeys(sks)
    table = bls.ValidatorKeyTable(pks)
    members = list(range(size))
    committee = table.load_committee(0, members)
    pats = []
    for s in range(n):
        chosen = set(random.Random(1000 + s).sample(range(size), a.participants))
        pats.append([i in chosen for i in range(size)])
    msgs = [synth.bench_message(2, s) for s in range(n)]
    agg = [sum(sks[i] for i in range(size) if p[i]) % synth.R_ORDER for p in pats]
    blob = synth.sign_blob(agg, msgs)
    sigs = [blob[96 * s : 96 * s + 96] for s in range(n)]

    keep = []

    def cbuf(b):
        buf = ctypes.create_string_buffer(bytes(b), max(1, len(b)))
        keep.append(buf)
        return ctypes.cast(buf, ctypes.c_void_p)

    by_bytes = synth.SetArray.from_lists([[pks[i] for i in range(size) if p[i]] for p in pats], msgs, sigs)
    idx_arr = (native.TblsSetIdx * n)()
    bits_arr = (native.TblsSetBits * n)()
    for s, p in enumerate(pats):
        ids = [i for i in range(size) if p[i]]
        ib = (ctypes.c_uint32 * len(ids))(*ids)
        keep.append(ib)
        row = bytearray((size + 7) // 8)
        for i in ids:
            row[i // 8] |= 1 << (i % 8)
        m, sg = cbuf(msgs[s]), cbuf(sigs[s])
        idx_arr[s].key_idx, idx_arr[s].n_pks = ctypes.cast(ib, ctypes.c_void_p), len(ids)
        idx_arr[s].msg, idx_arr[s].msg_len, idx_arr[s].sig = m, len(msgs[s]), sg
        bits_arr[s].bits, bits_arr[s].msg, bits_arr[s].msg_len, bits_arr[s].sig = cbuf(row), m, len(msgs[s]), sg
    out = (ctypes.c_int * n)()
    paths = {
        "bytes": lambda: L.tbls_fast_aggregate_verify_many(by_bytes.ptr, n, out),
        "idx": lambda: L.tbls_fast_aggregate_verify_many_idx(idx_arr, n, out),
        "bits": lambda: L.tbls_fast_aggregate_verify_many_bits(committee.slot, bits_arr, n, out),
    }
    order = a.order.split(",")
    assert sorted(order) == sorted(paths), "--order names each path once"
    ms = {k: [] for k in order}
    for it in range(a.warmup + a.reps):
        for name in order:
            call = paths[name]
            t0 = time.perf_counter()
            rc = call()
            dt = time.perf_counter() - t0
            assert rc == native.SUCCESS and list(out) == [1] * n, (name, rc)
            if it >= a.warmup:
                ms[name].append(1e3 * dt)
    res = {
        "metric": "fastAggregateVerify of sync-committee sets, ms per call (host clock, p50)",
        "sets": n,
        "committee_size": size,
        "participants": a.participants,
        "reps": a.reps,
        "warmup": a.warmup,
        "order": a.order,
    }
    for name, v in ms.items():
        v.sort()
        res[f"{name}_p50_ms"] = round(statistics.median(v), 4)
        res[f"{name}_min_ms"] = round(v[0], 4)
        res[f"{name}_p90_ms"] = round(v[int(0.9 * (len(v) - 1))], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
