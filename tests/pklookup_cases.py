"""Inputs and runners of tests/test_gpu_pklookup.py (byte-keyed batches that
resolve known keys from the resident key table's index), shared between the
test process and the child processes it starts for the library settings that
are read once per process:

    python -m tests.pklookup_cases lookup_off        TBLS_PK_LOOKUP=0
    python -m tests.pklookup_cases two_devices N     two library devices on one GPU, N sets

A child prints one JSON line: the verdicts and the lookup counters of each
call.  The parent holds the expectations (the C oracle's verdicts, and the hit
and miss counts derived from the batch's layout).

The single-key batch: N_SINGLE = 600 sets (above the 512 sets up to which the
one-kernel key stage decodes keys itself).  77 sets carry a key outside the
table -- the first set, the last, and every 8th from set 3 -- so every
64-lane wave of the lookup holds hits and misses and the miss count is no
multiple of 64.  Set 100 carries the infinity key, set 200 BAD_PK (both in
TABLE, absent from TABLE_LACKING), set 300 a signature that belongs to set 301.
"""

import json
import sys

N_TAB = 300
N_OUT = 80
N_SINGLE = 600
MISS_POS = frozenset([0, N_SINGLE - 1] + [3 + 8 * k for k in range(75)])
P_INF, P_BAD, P_TAMPER = 100, 200, 300
X_GE_P = bytes([0x9F]) + b"\xff" * 47  # compressed, x >= p: TBLS_BAD_ENCODING
assert len(MISS_POS) == 77 and not MISS_POS & {P_INF, P_BAD, P_TAMPER, P_TAMPER + 1}


class World:
    """Keys, tables and batches (needs the initialised library: the keys and
    signatures are made on the GPU, teku_amd/synth.py)."""

    def __init__(self):
        from teku_amd import synth as S

        self.S = S
        self.sk_tab = [S.interop_sk(70000 + i) for i in range(N_TAB)]
        self.sk_out = [S.interop_sk(80000 + i) for i in range(N_OUT)]
        pk = S.pubkeys(self.sk_tab + self.sk_out)
        self.pk_tab, self.pk_out = pk[:N_TAB], pk[N_TAB:]
        # the table of the issue: 300 interop keys, the infinity key, BAD_PK, x >= p, a second copy of key 0
        self.TABLE = self.pk_tab + [S.INFINITY_G1, S.BAD_PK, X_GE_P, self.pk_tab[0]]
        self.TABLE_LACKING = self.pk_tab + [X_GE_P, self.pk_tab[0]]  # without the infinity key and BAD_PK
        self.TABLE_OTHER = list(self.pk_out)  # different keys: what TABLE knew is unknown here
        self.single = self._single(invalid=True)
        self.single_valid = self._single(invalid=False)
        self.multi = self._multi()

    def _single(self, invalid):
        S = self.S
        pk, sk = [], []
        j = 0
        for p in range(N_SINGLE):
            if p in MISS_POS:
                pk.append(self.pk_out[j])
                sk.append(self.sk_out[j])
                j += 1
            elif invalid and p in (P_INF, P_BAD):
                pk.append(S.INFINITY_G1 if p == P_INF else S.BAD_PK)
                sk.append(1)  # some valid signature: the key fails the set
            else:
                t = (7 * p) % N_TAB
                pk.append(self.pk_tab[t])
                sk.append(self.sk_tab[t])
        ms = [S.bench_message(51, p) for p in range(N_SINGLE)]
        blob = S.sign_blob(sk, ms)
        sg = [blob[96 * p : 96 * p + 96] for p in range(N_SINGLE)]
        if invalid:
            sg[P_TAMPER] = sg[P_TAMPER + 1]
        return pk, ms, sg

    def single_times(self, reps):
        """The single-key batch, or with reps > 1 its keys `reps` times over
        fresh messages (the same signers; set 300 again carries set 301's
        signature)."""
        if reps == 1:
            return self.single
        S = self.S
        n = reps * N_SINGLE
        pk = self.single[0] * reps
        sk_of = dict(zip(self.pk_tab + self.pk_out, self.sk_tab + self.sk_out))
        ms = [S.bench_message(53, p) for p in range(n)]
        blob = S.sign_blob([sk_of.get(k, 1) for k in pk], ms)
        sg = [blob[96 * p : 96 * p + 96] for p in range(n)]
        sg[P_TAMPER] = sg[P_TAMPER + 1]
        return pk, ms, sg

    def _multi(self):
        """3 sets x 40 keys: all from the table, none from it, 20 and 20 interleaved."""
        S = self.S
        pick = [
            [("t", 100 + k) for k in range(40)],
            [("o", k) for k in range(40)],
            [("t", 200 + k) if k % 2 == 0 else ("o", 40 + k) for k in range(40)],
        ]
        keys = [[(self.pk_tab if w == "t" else self.pk_out)[i] for w, i in ks] for ks in pick]
        agg = [sum((self.sk_tab if w == "t" else self.sk_out)[i] for w, i in ks) % S.R_ORDER for ks in pick]
        ms = [S.bench_message(52, s) for s in range(3)]
        blob = S.sign_blob(agg, ms)
        return keys, ms, [blob[96 * s : 96 * s + 96] for s in range(3)]

    def hits(self, keys, table):
        """(hits, misses) of one key stage over `keys` with `table` loaded."""
        known = set(table)
        h = sum(1 for k in keys if k in known)
        return h, len(keys) - h


RANDS_SEED = 0x51AB


def rands(W, n):
    import random

    return W.S.random_multipliers(n, random.Random(RANDS_SEED))


def run_single(W, batch, n=N_SINGLE):
    """The three byte-keyed calls over the first n sets of a single-key batch,
    the lookup counters read and reset after each:
    {call: {"ok" / "each": verdicts, "stats": [hits, misses]}}."""
    from teku_amd import bls

    pk, ms, sg = (x[:n] for x in batch)
    arr = W.S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [len(m) for m in ms], b"".join(sg))
    stats = lambda: list(bls.ValidatorKeyTable.lookup_stats(reset=True))  # noqa: E731
    stats()
    out = {}
    ok = arr.batch_verify(rands(W, n))
    out["batch_verify"] = {"ok": ok, "stats": stats()}
    each = arr.verify_each()
    out["verify_each"] = {"each": each, "stats": stats()}
    ok, each = arr.batch_verify_each(rands(W, n))
    out["batch_verify_each"] = {"ok": ok, "each": each, "stats": stats()}
    return out


def run_multi(W, sets):
    """tbls_fast_aggregate_verify_many (the per-set pass's key stage behind the
    batch's) and tbls_batch_verify (the batch pipeline's) over multi-key sets."""
    from teku_amd import bls

    keys, ms, sg = sets
    arr = W.S.SetArray.from_lists(keys, ms, sg)
    stats = lambda: list(bls.ValidatorKeyTable.lookup_stats(reset=True))  # noqa: E731
    stats()
    out = {}
    each = arr.fast_aggregate_verify_many()
    out["fast_aggregate_verify_many"] = {"each": each, "stats": stats()}
    ok = arr.batch_verify(rands(W, len(ms)))
    out["batch_verify"] = {"ok": ok, "stats": stats()}
    return out


def main():
    mode = sys.argv[1]
    import torch  # noqa: F401  (one HIP runtime: torch's, teku_amd/native.py)

    from teku_amd import bls, native

    if mode == "two_devices":
        L = native.load_library()
        native.check(L.tbls_init(2, 1), "tbls_init(share devices)")
        native._lib = L
    else:
        L = native.lib()
    W = World()
    out = {"devices": L.tbls_device_count()}
    table = bls.ValidatorKeyTable(W.TABLE)
    if mode == "lookup_off":
        out["single"] = run_single(W, W.single)
        out["multi"] = run_multi(W, W.multi)
        try:
            table.resolve(W.TABLE[:1])
            out["resolve"] = "answered"
        except ValueError:
            out["resolve"] = "ValueError"
    else:
        n = int(sys.argv[2])
        batch = W.single_times(n // N_SINGLE)
        t = native.TblsTiming()
        arr = W.S.SetArray(b"".join(batch[0]), [1] * n, b"".join(batch[1]), [32] * n, b"".join(batch[2]))
        table.lookup_stats(reset=True)
        ok = arr.batch_verify(rands(W, n), timing=t)
        out["batch_verify"] = {"ok": ok, "stats": list(table.lookup_stats(reset=True)), "n_devices": t.n_devices}
        te = native.TblsTiming()
        ok, each = arr.batch_verify_each(rands(W, n), timing=te)
        out["batch_verify_each"] = {"ok": ok, "each": each, "stats": list(table.lookup_stats(reset=True)), "n_devices": te.n_devices}
    table.clear()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
