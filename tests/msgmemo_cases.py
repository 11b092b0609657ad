"""Inputs of the hash-point memo's GPU tests (tests/test_gpu_msgmemo.py), and,
run as `python -m tests.msgmemo_cases <mode>`, the cases that need a process of
their own because the library reads the setting once (TBLS_MSG_MEMO,
TBLS_SHARD_MIN, the device count of tbls_init).  Prints `RESULT <json>`.

  two_devices     tbls_init(2, TBLS_INIT_SHARE_DEVICES) with TBLS_SHARD_MIN=300
                  and TBLS_MSG_MEMO=64 in the environment: 600 sets over 40
                  messages, set i signing message i mod 40, cut into two shards
                  of 300 that each hold all 40 messages; tbls_batch_verify
                  twice, then tbls_batch_verify_each with sets 10 and 590 bad
                  (both shards fail, and 300 sets re-stage to settle)
  off_env         TBLS_MSG_MEMO unset: the small batch's calls, nothing else
  off_configured  tbls_msg_memo_configure(4), one batch, then configure(0),
                  then the same calls
"""
import ctypes
import json
import os
import sys

THREADS = max(1, min(16, os.cpu_count() or 1))


def msg(tag, n=32):
    return bytes((tag * 37 + j * 11 + 5) & 0xFF for j in range(n))


def small_batches(S):
    """The 8-set batches of the small test: (keys, messages, signatures, bad set)
    -- 3 distinct 32-byte messages, the empty message, a 65-byte message and
    one tampered signature; then 8 valid sets over five new messages."""
    sks = [S.interop_sk(900 + i) for i in range(8)]
    pk = S.pubkeys(sks)
    a, b, c, empty, m65 = msg(1), msg(2), msg(3), b"", msg(4, 65)
    ms1 = [a, b, c, a, empty, m65, b, c]
    blob = S.sign_blob(sks, ms1)
    sg1 = [blob[96 * i : 96 * i + 96] for i in range(8)]
    sg1[7] = S.sign_blob([sks[7]], [a])  # set 7's key on another message
    n1, n2, n3, n4, n5 = (msg(10 + k) for k in range(5))
    ms3 = [n1, n2, n3, n4, n5, n1, n2, n3]
    blob = S.sign_blob(sks, ms3)
    sg3 = [blob[96 * i : 96 * i + 96] for i in range(8)]
    return pk, (ms1, sg1), (ms3, sg3)


def each(S, native, pk, ms, sg, r):
    """tbls_batch_verify_each on single-key sets: (rc, ok, verdicts)"""
    n = len(pk)
    arr = S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [len(x) for x in ms], b"".join(sg))
    rr = (ctypes.c_uint64 * n)(*r)
    ok, out = ctypes.c_int(-1), (ctypes.c_int * n)()
    rc = native.lib().tbls_batch_verify_each(arr.ptr, n, rr, 0, ctypes.byref(ok), out, None)
    return rc, ok.value, [v == 1 for v in out[:n]]


def memo_stats(native, reset=False):
    out = (ctypes.c_uint64 * 4)()
    native.check(native.lib().tbls_msg_memo_stats(out, 1 if reset else 0), "tbls_msg_memo_stats")
    return [int(x) for x in out]


def _small_calls(S, native):
    pk, (ms1, sg1), (ms3, sg3) = small_batches(S)
    r = list(range(3, 11))
    native.stats(reset=True)
    calls = [each(S, native, pk, ms1, sg1, r), each(S, native, pk, ms1, sg1, r), each(S, native, pk, ms3, sg3, r)]
    return {"calls": calls, "memo": memo_stats(native), "stats": native.stats()}


def main(mode):
    import torch  # noqa: F401  (one HIP runtime: torch's, teku_amd/native.py)

    from oracle import c_oracle as C
    from teku_amd import native, synth as S

    if mode == "two_devices":
        L = native.load_library()
        native.check(L.tbls_init(2, 1), "tbls_init(share devices)")
        native._lib = L
        n, m = 600, 40
        sks = [S.interop_sk(i) for i in range(n)]
        pk = S.pubkeys(sks)
        roots = [S.bench_message(41, g) for g in range(m)]
        ms = [roots[i % m] for i in range(n)]
        blob = S.sign_blob(sks, ms)
        sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
        r = S.random_multipliers(n)
        out = {"devices": L.tbls_device_count(), "calls": []}
        arr = S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [32] * n, b"".join(sg))
        for _ in range(2):
            t = native.TblsTiming()
            out["calls"].append({"ok": arr.batch_verify(r, timing=t), "n_devices": t.n_devices, "memo": memo_stats(native)})
        bad = [10, 590]
        for j in bad:
            sg[j] = sg[j + 1]
        exp = C.verify_each([[k] for k in pk], ms, sg, threads=THREADS)
        rc, ok, got = each(S, native, pk, ms, sg, r)
        out["each"] = {"rc": rc, "ok": ok, "failed": [i for i in range(n) if not got[i]], "expected": [i for i in range(n) if not exp[i]],
                       "memo": memo_stats(native)}
    elif mode == "off_env":
        native.lib()
        out = _small_calls(S, native)
    elif mode == "off_configured":
        L = native.lib()
        native.check(L.tbls_msg_memo_configure(4), "configure")
        pk, (ms1, sg1), _ = small_batches(S)
        each(S, native, pk, ms1, sg1, list(range(3, 11)))
        used = memo_stats(native)
        native.check(L.tbls_msg_memo_configure(0), "configure")
        out = _small_calls(S, native)
        out["used_before"] = used
    else:
        raise SystemExit("unknown mode " + mode)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
