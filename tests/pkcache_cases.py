"""Runners of tests/test_gpu_pkcache.py (the learned key cache of byte-keyed
batches) over the inputs of tests/pklookup_cases.py, shared
between the test process and the child processes it starts for the settings
that are read once per process:

    python -m tests.pkcache_cases record        tbls_dev_batch_partial's record, cold and warm (the parent sets TBLS_PK_CACHE=0)
    python -m tests.pkcache_cases small         three calls of each entry (the parent sets TBLS_PK_CACHE_KEYS=64)
    python -m tests.pkcache_cases lookup_off    the same (the parent sets TBLS_PK_LOOKUP=0)
    python -m tests.pkcache_cases two_devices   two library devices on one GPU, 1,200 sets, two calls

A child prints one JSON line; the parent holds the expectations.
"""

import ctypes
import json
import sys

from tests import pklookup_cases as K


def cache_stats(reset=True):
    """[hits, learned, refused, rows in use] of the learned caches, reset after reading."""
    from teku_amd import bls

    return list(bls.pk_cache_stats(reset=reset))


def lookup_stats():
    from teku_amd import bls

    return list(bls.ValidatorKeyTable.lookup_stats(reset=True))


def run_calls(W, batch, calls=("batch_verify", "verify_each", "batch_verify_each")):
    """The byte-keyed calls over a single-key batch, in order; after each, its
    verdicts, the cache counters and the table lookup counters (both reset):
    [{"call", "ok" / "each", "cache": [hits, learned, refused, rows], "lookup": [hits, misses]}]."""
    pk, ms, sg = batch
    n = len(pk)
    arr = W.S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [len(m) for m in ms], b"".join(sg))
    cache_stats()
    lookup_stats()
    out = []
    for call in calls:
        r = {"call": call}
        if call == "batch_verify":
            r["ok"] = arr.batch_verify(K.rands(W, n))
        elif call == "verify_each":
            r["each"] = arr.verify_each()
        else:
            r["ok"], r["each"] = arr.batch_verify_each(K.rands(W, n))
        r["cache"] = cache_stats()
        r["lookup"] = lookup_stats()
        out.append(r)
    return out


def eight_key_batch(W):
    """600 single-key sets over 8 distinct valid keys (set p: table key p mod 8), all valid."""
    S = W.S
    n = K.N_SINGLE
    pk = [W.pk_tab[p % 8] for p in range(n)]
    ms = [S.bench_message(54, p) for p in range(n)]
    blob = S.sign_blob([W.sk_tab[p % 8] for p in range(n)], ms)
    return pk, ms, [blob[96 * p : 96 * p + 96] for p in range(n)]


class DevPartial:
    """tbls_dev_batch_partial + tbls_dev_final_verify of a single-key batch whose inputs lie in device memory."""

    def __init__(self, W, batch):
        import torch

        from teku_amd import native

        self.torch, self.native = torch, native
        pk, ms, sg = batch
        n = self.n = len(pk)
        self.dev = torch.device("cuda", 0)
        u8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(self.dev)  # noqa: E731
        rr = K.rands(W, n)
        self.bufs = dict(pks=u8(b"".join(pk)), msgs=u8(b"".join(ms)), sigs=u8(b"".join(sg)),
                         pk_off=torch.arange(0, n + 1, dtype=torch.int32, device=self.dev),
                         msg_off=torch.arange(0, 32 * (n + 1), 32, dtype=torch.int32, device=self.dev),
                         rand=torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in rr], dtype=torch.int64, device=self.dev))
        b = self.bufs
        self.desc = native.TblsDevBatch(b["pks"].data_ptr(), b["pk_off"].data_ptr(), n, b["msgs"].data_ptr(), b["msg_off"].data_ptr(),
                                        b["sigs"].data_ptr(), b["rand"].data_ptr(), n)

    def __call__(self):
        """(the 580-byte record as hex, the final verification's verdict)"""
        torch, native = self.torch, self.native
        L = native.lib()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        out = torch.zeros(native.PARTIAL_BYTES, dtype=torch.uint8, device=self.dev)
        native.check(L.tbls_dev_batch_partial(0, ctypes.byref(self.desc), stream, out.data_ptr()), "partial")
        ok = ctypes.c_int(7)
        native.check(L.tbls_dev_final_verify(0, out.data_ptr(), 1, stream, ctypes.byref(ok)), "final")
        torch.cuda.synchronize()
        return bytes(out.cpu().numpy()).hex(), ok.value


def main():
    mode = sys.argv[1]
    import torch  # noqa: F401  (one HIP runtime: torch's, teku_amd/native.py)

    from teku_amd import native

    if mode == "two_devices":
        L = native.load_library()
        native.check(L.tbls_init(2, 1), "tbls_init(share devices)")
        native._lib = L
    else:
        L = native.lib()
    W = K.World()
    out = {"devices": L.tbls_device_count()}
    if mode == "record":
        part = DevPartial(W, W.single_valid)
        cache_stats()
        out["records"] = []
        for _ in range(2):
            rec, ok = part()
            out["records"].append({"rec": rec, "ok": ok, "cache": cache_stats()})
    elif mode in ("small", "lookup_off"):
        out["rounds"] = [run_calls(W, W.single) for _ in range(2)]
    else:
        batch = W.single_times(2)
        n = len(batch[0])
        arr = W.S.SetArray(b"".join(batch[0]), [1] * n, b"".join(batch[1]), [32] * n, b"".join(batch[2]))
        cache_stats()
        out["calls"] = []
        for _ in range(2):
            t = native.TblsTiming()
            ok = arr.batch_verify(K.rands(W, n), timing=t)
            out["calls"].append({"ok": ok, "n_devices": t.n_devices, "cache": cache_stats()})
        out["each"] = arr.verify_each()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
