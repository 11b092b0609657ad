"""Byte-keyed batches with and without the key table's index:
three shapes, five legs each, on one build.

  shapes  cfg2   64 sets x 512 keys       tbls_fast_aggregate_verify_many
          cfg4   16,384 single-key sets   tbls_batch_verify_each
          131k   131,072 single-key sets  tbls_dev_batch_partial + the final verification
  legs    a  byte keys, no table
          b  byte keys, the table holds every key of the batch
          c  byte keys, a table of the same size that holds none of them
          d  the index entry point, where one exists (cfg2:
             tbls_fast_aggregate_verify_many_idx, 131k: tbls_dev_batch_partial_idx)
          e  as b with TBLS_PK_LOOKUP=0, in a child process (the setting is
             read once per process)

The table state differs between a, c and b/d, so the legs run in phases (no
table; the disjoint table; the full table), and the phases repeat --rounds
times so that drift over the run shows up inside every leg.  Within a phase
the shapes' calls are interleaved.  Every call is timed on the host clock
around a call that ends in a device synchronise; a leg's figure is the p50 of
its --rounds x --reps calls after --warmup calls per phase.  The table loads
are timed the same way (with the index build here, without it in the child).
Writes one JSON object to --out and prints it."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_TABLE = 65536  # interop keys [0, 65536): every key of the three shapes
OTHER_FIRST = 1000000  # the disjoint table: interop keys [1000000, 1065536)


def p50(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per leg at the start of every phase")
    ap.add_argument("--n-big", type=int, default=131072)
    ap.add_argument("--child", action="store_true", help="leg e: run by this tool itself with TBLS_PK_LOOKUP=0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pk_lookup.json"))
    a = ap.parse_args()
    import torch

    from teku_amd import bls, native, synth

    L = native.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t_gen = time.perf_counter()
    tab_keys = synth.pubkeys([synth.interop_sk(i) for i in range(N_TABLE)])
    other_keys = None if a.child else synth.pubkeys([synth.interop_sk(OTHER_FIRST + i) for i in range(N_TABLE)])

    # cfg2: set s holds interop keys [512 s, 512 s + 512)
    keys2, msgs2, sigs2 = synth.multi_key(64, 512)
    assert keys2[63][511] == tab_keys[64 * 512 - 1]
    arr2 = synth.SetArray.from_lists(keys2, msgs2, sigs2)
    keep = []
    idx2 = (native.TblsSetIdx * 64)()
    for s in range(64):
        ib = (ctypes.c_uint32 * 512)(*range(512 * s, 512 * s + 512))
        mb, sb = ctypes.create_string_buffer(msgs2[s], 32), ctypes.create_string_buffer(sigs2[s], 96)
        keep += [ib, mb, sb]
        idx2[s].key_idx, idx2[s].n_pks = ctypes.cast(ib, ctypes.c_void_p), 512
        idx2[s].msg, idx2[s].msg_len, idx2[s].sig = ctypes.cast(mb, ctypes.c_void_p), 32, ctypes.cast(sb, ctypes.c_void_p)
    out2 = (ctypes.c_int * 64)()

    # cfg4: set j is signed by interop key j
    n4 = 16384
    pk4, ms4, sg4 = synth.single_signer(0, n4, seed=4)
    arr4 = synth.SetArray.single(pk4, ms4, sg4)
    each4 = (ctypes.c_int * n4)()
    ok = ctypes.c_int(0)

    # 131k: set j is signed by interop key j mod 65536; inputs in HBM
    nb = a.n_big
    pkb, msb, sgb = synth.single_signer(0, nb)
    u8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    big = dict(pks=u8(pkb), msgs=u8(msb), sigs=u8(sgb), pk_off=torch.arange(0, nb + 1, dtype=torch.int32, device=dev),
               msg_off=torch.arange(0, 32 * (nb + 1), 32, dtype=torch.int32, device=dev),
               rand=torch.from_numpy(synth.fast_multipliers(nb).view("int64")).to(dev),
               key_idx=(torch.arange(0, nb, dtype=torch.int32, device=dev) % N_TABLE).contiguous())
    desc = native.TblsDevBatch(big["pks"].data_ptr(), big["pk_off"].data_ptr(), nb, big["msgs"].data_ptr(), big["msg_off"].data_ptr(),
                               big["sigs"].data_ptr(), big["rand"].data_ptr(), nb)
    rec = torch.empty(native.PARTIAL_BYTES, dtype=torch.uint8, device=dev)
    gen_s = time.perf_counter() - t_gen

    def call_cfg2():
        assert L.tbls_fast_aggregate_verify_many(arr2.ptr, 64, out2) == native.SUCCESS and list(out2) == [1] * 64

    def call_cfg2_idx():
        assert L.tbls_fast_aggregate_verify_many_idx(idx2, 64, out2) == native.SUCCESS and list(out2) == [1] * 64

    def call_cfg4():
        rr = synth.fast_multipliers(n4)
        rc = L.tbls_batch_verify_each(arr4.ptr, n4, rr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, ctypes.byref(ok), each4, None)
        assert rc == native.SUCCESS and ok.value == 1

    def final():
        assert L.tbls_dev_final_verify(0, rec.data_ptr(), 1, stream, ctypes.byref(ok)) == native.SUCCESS and ok.value == 1

    def call_big():
        assert L.tbls_dev_batch_partial(0, ctypes.byref(desc), stream, rec.data_ptr()) == native.SUCCESS
        final()

    def call_big_idx():
        assert L.tbls_dev_batch_partial_idx(0, ctypes.byref(desc), big["key_idx"].data_ptr(), stream, rec.data_ptr()) == native.SUCCESS
        final()

    byte_calls = {"cfg2": call_cfg2, "cfg4": call_cfg4, "131k": call_big}
    idx_calls = {"cfg2": call_cfg2_idx, "131k": call_big_idx}
    ms = {}
    load_ms = {}
    counts = {}

    def timed_load(name, keys):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = bls.ValidatorKeyTable(keys)
        load_ms.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
        return t

    def phase(leg, calls):
        for name, call in calls.items():
            for _ in range(a.warmup):
                call()
            bls.ValidatorKeyTable.lookup_stats(reset=True)
            call()
            counts[f"{name}_{leg}"] = list(bls.ValidatorKeyTable.lookup_stats(reset=True))  # one call's hits and misses
        for _ in range(a.reps):
            for name, call in calls.items():  # interleaved
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                ms.setdefault(f"{name}_{leg}", []).append(1e3 * (time.perf_counter() - t0))

    if a.child:
        for _ in range(a.rounds):
            timed_load("without_index", tab_keys)
            phase("e", byte_calls)
        res = {"ms": ms, "load_ms": load_ms, "counts": counts}
        print("CHILD " + json.dumps(res), flush=True)
        return

    for _ in range(a.rounds):
        L.tbls_pk_table_clear()
        phase("a", byte_calls)
        timed_load("with_index_other_keys", other_keys)
        phase("c", byte_calls)
        timed_load("with_index", tab_keys)
        phase("b", byte_calls)
        phase("d", idx_calls)
    L.tbls_pk_table_clear()
    torch.cuda.synchronize()
    env = dict(os.environ, TBLS_PK_LOOKUP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds), "--warmup",
                        str(a.warmup), "--n-big", str(nb)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    child = json.loads([x for x in r.stdout.splitlines() if x.startswith("CHILD ")][-1][6:])
    ms.update(child["ms"])
    load_ms.update(child["load_ms"])
    counts.update(child["counts"])

    res = {
        "metric": "byte-keyed batches with the key table's index: ms per call (host clock around a blocking call, p50)",
        "shapes": {"cfg2": "64 x 512 keys, tbls_fast_aggregate_verify_many", "cfg4": "16,384 sets, tbls_batch_verify_each",
                   "131k": "%d sets, tbls_dev_batch_partial + tbls_dev_final_verify" % nb},
        "legs": {"a": "byte keys, no table", "b": "byte keys, table holds every key", "c": "byte keys, table of the same size holds none",
                 "d": "index entry point", "e": "b with TBLS_PK_LOOKUP=0 (child process)"},
        "table_keys": N_TABLE,
        "reps_per_leg": a.reps * a.rounds,
        "rounds": a.rounds,
        "warmup_per_phase": a.warmup,
        "workload_gen_s": round(gen_s, 2),
        "p50_ms": {k: p50(v) for k, v in sorted(ms.items())},
        "min_ms": {k: round(min(v), 4) for k, v in sorted(ms.items())},
        "p50_ms_by_round": {k: [p50(v[i * a.reps:(i + 1) * a.reps]) for i in range(a.rounds)] for k, v in sorted(ms.items())},
        "lookup_hits_misses_per_call": counts,
        "table_load_ms": {k: [round(x, 3) for x in v] for k, v in load_ms.items()},
    }
    q = res["p50_ms"]
    res["summary"] = {
        s: {"b_minus_a_ms": round(q[f"{s}_b"] - q[f"{s}_a"], 4), "c_over_a": round(q[f"{s}_c"] / q[f"{s}_a"], 4),
            "e_over_a": round(q[f"{s}_e"] / q[f"{s}_a"], 4),
            "d_minus_a_ms": round(q[f"{s}_d"] - q[f"{s}_a"], 4) if f"{s}_d" in q else None}
        for s in byte_calls
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
