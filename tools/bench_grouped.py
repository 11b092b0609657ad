"""Grouped batches against ungrouped ones on device-resident inputs: n
single-key sets that sign m distinct messages (set i signs message i mod m),
through tbls_dev_batch_partial_grouped + tbls_dev_final_verify and through
tbls_dev_batch_partial + tbls_dev_final_verify on the same sets with the same
randomizers.  Each call is timed on the host clock around work that ends in
the final verification's synchronise; per shape, after `warmup` calls of each
path, the two paths alternate for `reps` timed calls each, and the p50 / min /
p90 are reported in ms.  The ungrouped path's exclusive stage times come from
tbls_dev_batch_stage_profile (the grouped launch has no stage-profile entry).

    python tools/bench_grouped.py [--reps 15] [--warmup 3] [--out profiles/grouped.json] [--quick]

Shapes: 16,384 sets with m in {1, 64, 2,048, 16,384}; 131,072 sets with m in
{64, 2,048}; and the sweep behind tb_plan.h's TB_GROUP_MIN / TB_GROUP_PERCENT:
n in {128, 512, 2,048, 8,192} at m = n / 64 and m = n / 2.  m == n is not a
grouped launch: that row times the ungrouped path only.  Writes one JSON file.
"""

import argparse
import ctypes
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16384, 1), (16384, 64), (16384, 2048), (16384, 16384), (131072, 64), (131072, 2048)]
SWEEP = [(n, m) for n in (128, 512, 2048, 8192) for m in (n // 64, n // 2)]
STAGES = ("pk_decompress", "set_pk", "set_sig", "set_hash", "g2_sum", "miller", "prod")


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped.json"))
    ap.add_argument("--quick", action="store_true", help="the sweep's two smallest shapes only (a rehearsal)")
    a = ap.parse_args()

    import torch

    from teku_amd import native, synth

    L = native.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    u8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int64).to(torch.int32).to(dev)  # noqa: E731
    shapes = SWEEP[:2] if a.quick else SHAPES + SWEEP
    n_max = max(n for n, _ in shapes)
    n_keys = min(n_max, 65536)
    sks = [synth.interop_sk(i) for i in range(n_keys)]
    pk_list = synth.pubkeys(sks)
    rows = []
    for n, m in shapes:
        roots = [synth.bench_message(41, g) for g in range(m)]
        set_sk = [sks[i % n_keys] for i in range(n)]
        sigs = u8(synth.sign_blob(set_sk, [roots[i % m] for i in range(n)]))
        keys = u8(b"".join(pk_list[i % n_keys] for i in range(n)))
        pk_off = i32(list(range(n + 1)))
        r = synth.random_multipliers(n)
        rand = torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in r], dtype=torch.int64, device=dev)
        msgs_u, off_u = u8(b"".join(roots[i % m] for i in range(n))), i32([32 * i for i in range(n + 1)])
        msgs_g, off_g = u8(b"".join(roots)), i32([32 * g for g in range(m + 1)])
        per = [len(range(g, n, m)) for g in range(m)]
        grp_off = i32([0] + list(itertools.accumulate(per)))
        grp_sets = i32([i for g in range(m) for i in range(g, n, m)])
        plain = native.TblsDevBatch(keys.data_ptr(), pk_off.data_ptr(), n, msgs_u.data_ptr(), off_u.data_ptr(), sigs.data_ptr(), rand.data_ptr(), n)
        grouped = native.TblsDevBatch(keys.data_ptr(), pk_off.data_ptr(), n, msgs_g.data_ptr(), off_g.data_ptr(), sigs.data_ptr(), rand.data_ptr(), n)
        rec = torch.zeros(native.PARTIAL_BYTES, dtype=torch.uint8, device=dev)
        ok = ctypes.c_int(-1)

        def run_plain():
            native.check(L.tbls_dev_batch_partial(0, ctypes.byref(plain), stream, rec.data_ptr()), "partial")
            native.check(L.tbls_dev_final_verify(0, rec.data_ptr(), 1, stream, ctypes.byref(ok)), "final")
            assert ok.value == 1, "ungrouped batch rejected"

        def run_grouped():
            native.check(L.tbls_dev_batch_partial_grouped(0, ctypes.byref(grouped), None, m, grp_off.data_ptr(), grp_sets.data_ptr(), stream,
                                                          rec.data_ptr()), "partial_grouped")
            native.check(L.tbls_dev_final_verify(0, rec.data_ptr(), 1, stream, ctypes.byref(ok)), "final")
            assert ok.value == 1, "grouped batch rejected"

        paths = {"ungrouped": run_plain}
        if m < n:
            paths["grouped"] = run_grouped
        for fn in paths.values():
            for _ in range(a.warmup):
                fn()
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, fn in paths.items():
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        stage = (ctypes.c_float * 7)()
        native.check(L.tbls_dev_batch_stage_profile(0, ctypes.byref(plain), stream, rec.data_ptr(), stage), "stage_profile")
        row = {"n": n, "m": m, "group_plan": list(native.group_plan(n, m)),
               "ungrouped_stage_ms_exclusive": {k: round(float(v), 4) for k, v in zip(STAGES, stage)}}
        for k, xs in times.items():
            row[k + "_ms"] = {"p50": round(pct(xs, 0.5), 4), "min": round(min(xs), 4), "p90": round(pct(xs, 0.9), 4)}
        if "grouped" in times:
            row["speedup_p50"] = round(pct(times["ungrouped"], 0.5) / pct(times["grouped"], 0.5), 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"tool": "tools/bench_grouped.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "timing": "host clock around partial + final verification (synchronised), ms; paths alternate per repetition",
           "sets": "single-key sets, interop keys cyclic over %d, set i signs message i mod m, keys as bytes" % n_keys,
           "shapes": [r_ for r_ in rows if (r_["n"], r_["m"]) in SHAPES], "sweep": [r_ for r_ in rows if (r_["n"], r_["m"]) in SWEEP]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
