"""The hash-point memo at the host entries: ms per call of
tbls_batch_verify on n single-key sets given as bytes over m distinct
messages, and of tbls_batch_verify_each with 4 bad sets, in four legs per
shape, all in one process:

    off_a   the memo off (tbls_msg_memo_configure(0))
    cold    the memo on, tbls_msg_memo_clear before every timed call (untimed):
            every message is hashed, found new and learned
    warm    the memo on and every message resident
    off_b   the memo off again: off_a against off_b is the memo-off spread

Each leg is `--reps` calls one after another (the legs run as blocks, so that
no timed call pays for a row buffer's allocation: configure drops the rows);
the figure is the p50 of the host clock around the blocking call.  Shapes with
every message distinct, which the memo cannot help, include 131,072 sets, where
only the host-side grouping differs between off and cold.

    python tools/bench_msgmemo.py --out profiles/msgmemo.json
"""

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

SHAPES = [(128, 64, 0), (250, 64, 0), (2048, 64, 0), (16384, 64, 0), (16384, 2048, 0), (16384, 16384, 0), (16384, 64, 4), (131072, 131072, 0)]
KEYS = 4096  # distinct signers, cyclic over the sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and shape")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per leg and shape")
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--max-n", type=int, default=131072, help="leave out larger shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msgmemo.json"))
    a = ap.parse_args()
    import torch

    from teku_amd import bls, native, synth

    L = native.lib()
    sks = [synth.interop_sk(i) for i in range(KEYS)]
    keys = synth.pubkeys(sks)
    ok = ctypes.c_int(0)
    res = {
        "metric": "host entries with the hash-point memo: ms per call (host clock around a blocking call), p50 / min / max of calls_per_leg calls",
        "legs": {"off_a": "memo off", "cold": "memo on, cleared before each call (untimed)", "warm": "memo on, every message resident",
                 "off_b": "memo off again (the memo-off spread)"},
        "rows": a.rows, "calls_per_leg": a.reps, "shapes": {},
    }
    for n, m, n_bad in SHAPES:
        if n > a.max_n:
            continue
        name = "%d_over_%d%s" % (n, m, "_each_%dbad" % n_bad if n_bad else "")
        roots = [synth.bench_message(51, g) for g in range(m)]
        ms = [roots[i % m] for i in range(n)]
        blob = synth.sign_blob([sks[i % KEYS] for i in range(n)], ms)
        sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
        bad = [(k + 1) * n // (n_bad + 1) - 1 for k in range(n_bad)]
        for j in bad:
            sg[j] = sg[j - 1]
        arr = synth.SetArray(b"".join(keys[i % KEYS] for i in range(n)), [1] * n, b"".join(ms), [32] * n, b"".join(sg))
        each = (ctypes.c_int * n)()

        def call():
            rr = synth.fast_multipliers(n).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            if n_bad:
                rc = L.tbls_batch_verify_each(arr.ptr, n, rr, 1, ctypes.byref(ok), each, None)
                assert rc == native.SUCCESS and ok.value == 0
            else:
                assert L.tbls_batch_verify(arr.ptr, n, rr, 1, ctypes.byref(ok), None) == native.SUCCESS and ok.value == 1

        def leg(kind):
            bls.msg_memo_configure(0 if kind.startswith("off") else a.rows)
            for _ in range(a.warmup):
                call()
            if n_bad:  # the verdicts, outside the timed calls
                assert [i for i in range(n) if not each[i]] == bad
            times = []
            for _ in range(a.reps):
                if kind == "cold":
                    bls.msg_memo_clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                times.append(1e3 * (time.perf_counter() - t0))
            counters = bls.msg_memo_stats(reset=True)
            return {"p50_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
                    "counters": list(counters)}

        legs = ["off_a", "cold", "off_b"] if m == n else ["off_a", "cold", "warm", "off_b"]
        out = {k: leg(k) for k in legs}
        out["off_spread_ms"] = round(abs(out["off_a"]["p50_ms"] - out["off_b"]["p50_ms"]), 4)
        res["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    bls.msg_memo_configure(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
