"""Byte-keyed batches with the learned key cache: three shapes,
warm and cold, on one build.

  shapes  cfg2   64 sets x 512 keys       tbls_fast_aggregate_verify_many
          cfg4   16,384 single-key sets   tbls_batch_verify_each
          131k   131,072 single-key sets  tbls_dev_batch_partial + the final verification
  legs    warm   the cache holds every key of the batch (steady state)
          cold   tbls_pk_cache_clear before every call, outside the timed
                 region: every key misses, is decompressed and is learned

A build without the cache (the parent commit, or TBLS_PK_CACHE=0) runs the
same calls; its two legs are then the same measurement twice, which is its
run-to-run spread.  The legs alternate call by call, the shapes are
interleaved, and the rounds repeat so that drift shows up inside every leg.
Every call is timed on the host clock around a call that ends in a device
synchronise; a leg's figure is the p50 of its --rounds x --reps calls.
Writes one JSON object to --out and prints it."""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed calls per leg, shape and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per shape")
    ap.add_argument("--n-big", type=int, default=131072)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pk_learn_tool.json"))
    a = ap.parse_args()
    import torch

    from teku_amd import native, synth

    L = native.lib()
    has_cache = "tbls_pk_cache_clear" in native.EXPORTED
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    keys2, msgs2, sigs2 = synth.multi_key(64, 512)
    arr2 = synth.SetArray.from_lists(keys2, msgs2, sigs2)
    out2 = (ctypes.c_int * 64)()
    n4 = 16384
    pk4, ms4, sg4 = synth.single_signer(0, n4, seed=4)
    arr4 = synth.SetArray.single(pk4, ms4, sg4)
    each4 = (ctypes.c_int * n4)()
    ok = ctypes.c_int(0)
    nb = a.n_big
    pkb, msb, sgb = synth.single_signer(0, nb)
    u8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    big = dict(pks=u8(pkb), msgs=u8(msb), sigs=u8(sgb), pk_off=torch.arange(0, nb + 1, dtype=torch.int32, device=dev),
               msg_off=torch.arange(0, 32 * (nb + 1), 32, dtype=torch.int32, device=dev),
               rand=torch.from_numpy(synth.fast_multipliers(nb).view("int64")).to(dev))
    desc = native.TblsDevBatch(big["pks"].data_ptr(), big["pk_off"].data_ptr(), nb, big["msgs"].data_ptr(), big["msg_off"].data_ptr(),
                               big["sigs"].data_ptr(), big["rand"].data_ptr(), nb)
    rec = torch.empty(native.PARTIAL_BYTES, dtype=torch.uint8, device=dev)

    def call_cfg2():
        assert L.tbls_fast_aggregate_verify_many(arr2.ptr, 64, out2) == native.SUCCESS and list(out2) == [1] * 64

    def call_cfg4():
        rr = synth.fast_multipliers(n4)
        rc = L.tbls_batch_verify_each(arr4.ptr, n4, rr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, ctypes.byref(ok), each4, None)
        assert rc == native.SUCCESS and ok.value == 1

    def call_big():
        assert L.tbls_dev_batch_partial(0, ctypes.byref(desc), stream, rec.data_ptr()) == native.SUCCESS
        assert L.tbls_dev_final_verify(0, rec.data_ptr(), 1, stream, ctypes.byref(ok)) == native.SUCCESS and ok.value == 1

    calls = {"cfg2": call_cfg2, "cfg4": call_cfg4, "131k": call_big}
    ms = {}
    counts = {}

    def stats():
        out = (ctypes.c_uint64 * 4)()
        assert L.tbls_pk_cache_stats(out, 1) == native.SUCCESS
        return list(out)

    def timed(name, leg, call):
        if leg == "cold" and has_cache:
            assert L.tbls_pk_cache_clear() == native.SUCCESS
        elif leg == "warm" and has_cache:
            call()  # a cold call of another shape may have come between: learn this shape's keys again,
            call()  # and let the library see a call without misses (it orders the next call's stages by that)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.setdefault(f"{name}_{leg}", []).append(1e3 * (time.perf_counter() - t0))

    for name, call in calls.items():
        for _ in range(a.warmup):
            call()
        if has_cache:  # one cold and one warm call's counters: [hits, learned, refused, rows in use]
            assert L.tbls_pk_cache_clear() == native.SUCCESS
            call()
            counts[f"{name}_cold"] = stats()
            call()
            counts[f"{name}_warm"] = stats()
    for _ in range(a.rounds):
        for _ in range(a.reps):
            for leg in ("warm", "cold"):
                for name, call in calls.items():
                    timed(name, leg, call)

    p50 = lambda v: round(statistics.median(v), 4)  # noqa: E731
    res = {
        "metric": "byte-keyed batches with the learned key cache: ms per call (host clock around a blocking call, p50)",
        "shapes": {"cfg2": "64 x 512 keys, tbls_fast_aggregate_verify_many", "cfg4": "16,384 sets, tbls_batch_verify_each",
                   "131k": "%d sets, tbls_dev_batch_partial + tbls_dev_final_verify" % nb},
        "legs": {"warm": "every key in the cache", "cold": "tbls_pk_cache_clear before the call (untimed)"},
        "cache": has_cache and os.environ.get("TBLS_PK_CACHE") != "0" and os.environ.get("TBLS_PK_LOOKUP") != "0",
        "calls_per_leg": a.reps * a.rounds,
        "p50_ms": {k: p50(v) for k, v in sorted(ms.items())},
        "min_ms": {k: round(min(v), 4) for k, v in sorted(ms.items())},
        "max_ms": {k: round(max(v), 4) for k, v in sorted(ms.items())},
        "p50_ms_by_round": {k: [p50(v[i * a.reps:(i + 1) * a.reps]) for i in range(a.rounds)] for k, v in sorted(ms.items())},
        "cache_counters_per_call": counts,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
