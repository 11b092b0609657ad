"""A failed grouped batch's per-set verdicts, three ways, through the host
entries: n single-key sets (keys as bytes, no key table) that sign m distinct
messages (set i signs message i mod m), 4 sets with a bad signature at fixed
positions.  On one device (n_gpus = 1), per shape, after `warmup` calls of
each variant the variants alternate for `reps` timed calls each (host clock
around the call), and p50 / min / p90 are reported in ms:

  a   the two-call sequence: tbls_batch_verify_grouped, and as it fails,
      tbls_batch_verify_each on the same sets
  a2  the same sequence again: a's run-to-run spread
  b   tbls_batch_verify_each alone
  c   tbls_batch_verify_each_grouped

and with no bad set, the happy path: tbls_batch_verify_grouped (g) against
tbls_batch_verify_each_grouped (c), which must cost the same.  The grouped
entries run without TBLS_GROUP_FORCE where the thresholds group the shape, with
it otherwise (16,384 sets over 2,048 messages).  Every variant's verdicts are
checked against the bad positions before the timing.  Also recorded: the
tbls_timing total_ms / device_ms of variant c's and b's last call.

    python tools/bench_grouped_each.py [--reps 20] [--warmup 5] [--out profiles/grouped_each.json] [--quick]
    python tools/bench_grouped_each.py --trace 16384,64 [--reps 10]     (variant c only, for a kernel trace)
"""

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 16), (16384, 64), (16384, 2048), (131072, 64)]


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def summary(xs):
    return {"p50": round(pct(xs, 0.5), 4), "min": round(min(xs), 4), "p90": round(pct(xs, 0.9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_each.json"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape only (a rehearsal)")
    ap.add_argument("--trace", default=None, help="n,m: run variant c alone on this shape `reps` times and write nothing")
    a = ap.parse_args()

    import numpy as np
    import torch

    from teku_amd import native, synth

    L = native.lib()
    shapes = [tuple(int(x) for x in a.trace.split(","))] if a.trace else SHAPES[:1] if a.quick else SHAPES
    n_keys = min(max(n for n, _ in shapes), 65536)
    sks = [synth.interop_sk(i) for i in range(n_keys)]
    pk_list = synth.pubkeys(sks)
    rows = []
    for n, m in shapes:
        roots = [synth.bench_message(43, g) for g in range(m)]
        set_sk = [sks[i % n_keys] for i in range(n)]
        msgs = [roots[i % m] for i in range(n)]
        good = synth.sign_blob(set_sk, msgs)
        bad_at = [0, n // 3, n // 2 + 1, n - 1]
        bad = bytearray(good)
        for j in bad_at:
            k = (j + 1) % n  # another key's signature on another message
            bad[96 * j : 96 * j + 96] = good[96 * k : 96 * k + 96]
        keys, mbytes = b"".join(pk_list[i % n_keys] for i in range(n)), b"".join(msgs)
        arrs = {"bad": synth.SetArray(keys, [1] * n, mbytes, [32] * n, bytes(bad)), "good": synth.SetArray(keys, [1] * n, mbytes, [32] * n, good)}
        rands = np.array(synth.random_multipliers(n), dtype=np.uint64)
        rr = rands.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        flags = 0 if native.group_plan(n, m)[0] == 2 else native.GROUP_FORCE
        ok = ctypes.c_int(-1)
        each = (ctypes.c_int * n)()
        tim = {"b": native.TblsTiming(), "c": native.TblsTiming()}

        def grouped(arr):
            native.check(L.tbls_batch_verify_grouped(arr.ptr, n, rr, 1, flags, ctypes.byref(ok), None), "grouped")
            return ok.value

        def plain_each(arr):
            native.check(L.tbls_batch_verify_each(arr.ptr, n, rr, 1, ctypes.byref(ok), each, ctypes.byref(tim["b"])), "each")
            return ok.value

        def each_grouped(arr):
            native.check(L.tbls_batch_verify_each_grouped(arr.ptr, n, rr, 1, flags, ctypes.byref(ok), each, ctypes.byref(tim["c"])), "each_grouped")
            return ok.value

        def seq_a(arr):
            return grouped(arr) or plain_each(arr)

        def verdicts_ok(want_bad):
            return [i for i in range(n) if not each[i]] == sorted(want_bad)

        if a.trace:
            for _ in range(a.reps):
                assert each_grouped(arrs["bad"]) == 0 and verdicts_ok(bad_at)
            continue
        fail = {"a": seq_a, "a2": seq_a, "b": plain_each, "c": each_grouped}
        happy = {"g": grouped, "c": each_grouped}
        row = {"n": n, "m": m, "group_plan": list(native.group_plan(n, m)), "force": bool(flags), "bad_sets": bad_at}
        for label, arr, variants, want_bad in (("failed", arrs["bad"], fail, bad_at), ("valid", arrs["good"], happy, [])):
            st0 = native.stats()
            for k, fn in variants.items():
                for _ in range(a.warmup):
                    assert fn(arr) == (0 if want_bad else 1), (label, k)
                    if k != "g":
                        assert verdicts_ok(want_bad), (label, k)
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():
                    t0 = time.perf_counter()
                    fn(arr)
                    times[k].append((time.perf_counter() - t0) * 1e3)
            st1 = native.stats()
            row[label] = {k: summary(xs) for k, xs in times.items()}
            row[label]["stats_delta"] = {k: st1[k] - st0[k] for k in ("partials", "each_passes", "finals", "settled")}
            if label == "failed":
                pa, pa2, pc = pct(times["a"], 0.5), pct(times["a2"], 0.5), pct(times["c"], 0.5)
                row[label]["a_spread_ms"] = round(abs(pa - pa2), 4)
                row[label]["c_minus_a_ms"] = round(pc - min(pa, pa2), 4)
                row[label]["timing_last_call"] = {k: {"total_ms": round(t.total_ms, 4), "device_ms": round(t.device_ms, 4)} for k, t in tim.items()}
            else:
                row[label]["c_minus_g_ms"] = round(pct(times["c"], 0.5) - pct(times["g"], 0.5), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.trace:
        return
    out = {"tool": "tools/bench_grouped_each.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "timing": "host clock around each call (or sequence of calls), ms; the variants alternate per repetition; one device (n_gpus = 1)",
           "variants": {"a": "tbls_batch_verify_grouped then tbls_batch_verify_each", "a2": "a again (its spread)", "b": "tbls_batch_verify_each",
                        "c": "tbls_batch_verify_each_grouped", "g": "tbls_batch_verify_grouped"},
           "sets": "single-key sets, interop keys cyclic over %d, keys as bytes, no key table, set i signs message i mod m" % n_keys,
           "shapes": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
