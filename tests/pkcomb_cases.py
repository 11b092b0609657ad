"""Inputs and runners of tests/test_gpu_pkcomb.py (the per-key comb rows,
DESIGN.md 3n).

The kernel-level part: 130 sets over 131 keys for tests/native/k_test_pkcomb.hip.

The library-level part runs in child processes, because the settings it needs
are read once per process: the product takes a comb row only in the two-wave
key kernel, which batches reach from 32,768 sets, so the children run with
TBLS_W2_MIN=64 and TBLS_COOP=0 and reach it at 192 sets.

    python -m tests.pkcomb_cases     every step of the library-level check

The parent test runs it three times: as it is, with TBLS_PK_COMB_KEYS below
the key count, and with TBLS_PK_COMB=0; only the environment differs.  A child
prints one JSON line; the parent holds the expectations.
"""

import ctypes
import json
import random
import sys

M64 = (1 << 64) - 1
N_SETS, N_DISTINCT = 192, 64
BAD_SET = 77  # the set whose signature is another set's


def column(d, j):
    """The scalar whose comb digit is d in column j and zero elsewhere (tb_pkcomb.h comb_digit)."""
    return sum(1 << (16 * t + j) for t in range(4) if d >> t & 1)


def comb_scalars(count, seed=61):
    """tests/native/pkcomb_check.cpp's list: the edges, a scalar with three
    zero top teeth, one with zero digits in columns 15 and 0, sixteen whose
    walks start at every entry 1..15, then seeded random ones up to `count`."""
    rng = random.Random(seed)
    v = [1, 2, 1 << 15, 1 << 16, (1 << 16) + 1, 1 << 48, 1 << 63, M64, 0xBEEF, 0x7FFE7FFE7FFE7FFE]
    for d in range(1, 16):
        low = rng.getrandbits(64) & (((1 << d) - 1) * 0x0001000100010001)
        v.append(column(d, d) | low)
    v.append(column(15, 0))
    while len(v) < count:
        v.append(rng.getrandbits(64) or 1)
    return v[:count]


def first_entry(r):
    """The comb entry that starts r's walk."""
    for j in range(15, -1, -1):
        d = sum(((r >> (16 * t + j)) & 1) << t for t in range(4))
        if d:
            return d
    return 0


def kernel_batch():
    """(KeyBatch, modes, key_idx): 130 sets -- two full 64-lane workgroups and a
    partial one -- over 131 distinct keys.  Set 5 carries a key outside G1
    (pk_code != TB_SUCCESS), set 9 has r = 0, set 70 is a two-key aggregate; the
    others are single valid keys with comb_scalars.  modes[j] (per key): the
    first wave mixes not ready / the cache's row / the table's row lane by
    lane, the rest alternate cache and table with a few not ready.  key_idx:
    the by-index form of the same sets over a table that is the key list
    itself (the identity), so one reference serves both forms."""
    from oracle.keys import interop_sk
    from tests import stage_cases as S

    rs = comb_scalars(130)
    sets = []
    for i in range(130):
        sk = interop_sk(3000 + i)
        if i == 5:
            sets.append(S.KeySet([S.invalid_key("outside G1")], [None], rs[i], "outside G1"))
        elif i == 9:
            sets.append(S.KeySet([S.pk_of(sk)], [sk], 0, "r == 0"))
        elif i == 70:
            sk2 = interop_sk(3500)
            sets.append(S.KeySet([S.pk_of(sk), S.pk_of(sk2)], [sk, sk2], rs[i], "two keys"))
        else:
            sets.append(S.KeySet([S.pk_of(sk)], [sk], rs[i], "entry %d first" % first_entry(rs[i])))
    batch = S.key_batch(sets)
    assert batch.n_keys == 131 and len(set(batch.blob[48 * k : 48 * k + 48] for k in range(131))) == 131
    modes = [j % 3 if j < 64 else (0 if j % 11 == 0 else 1 + j % 2) for j in range(batch.n_keys)]
    return batch, modes, list(range(batch.n_keys))


def kernel_reference(batch):
    """Per set (P, code) as stage_set_pk defines them, from oracle/bls12_381.py:
    P = affine([r] sum of the keys), (0, 0) with TB_PK_IS_INFINITY for an
    invalid key or r == 0 (tests/stage_cases.py key_reference without the
    signature pairs' -[r] g1, which r == 0 has none of)."""
    from oracle import bls12_381 as O
    from tests import stage_cases as S

    out = []
    for i, r in enumerate(batch.rands):
        code, acc = O.SUCCESS, O.jac_inf(O.FP)
        for k in range(batch.pk_off[i], batch.pk_off[i + 1]):
            kc, a = O.pk_decode_validate(batch.blob[48 * k : 48 * k + 48])
            if kc != O.SUCCESS:
                code = O.PK_IS_INFINITY
                break
            acc = O.jac_add(O.FP, acc, O.jac_from_affine(O.FP, a))
        pt = O.jac_to_affine(O.FP, O.jac_mul(O.FP, acc, r)) if code == O.SUCCESS and r else None
        if pt is None:
            code = O.PK_IS_INFINITY
        out.append((pt or S.ZERO_G1, code))
    return out


# ---- library level ---------------------------------------------------------------
CHILD_ENV = {"TBLS_W2_MIN": "64", "TBLS_COOP": "0"}


class World:
    """192 single-key sets over 64 distinct keys (set p: key p mod 64), valid;
    `bad`: the same with set BAD_SET carrying its neighbour's signature."""

    def __init__(self):
        from teku_amd import synth as S

        self.S = S
        self.sk = [S.interop_sk(90000 + i) for i in range(N_DISTINCT)]
        self.pk = S.pubkeys(self.sk)
        pk = [self.pk[p % N_DISTINCT] for p in range(N_SETS)]
        ms = [S.bench_message(61, p) for p in range(N_SETS)]
        blob = S.sign_blob([self.sk[p % N_DISTINCT] for p in range(N_SETS)], ms)
        sg = [blob[96 * p : 96 * p + 96] for p in range(N_SETS)]
        self.good = (pk, ms, sg)
        bad = list(sg)
        bad[BAD_SET] = sg[BAD_SET + 1]
        self.bad = (pk, ms, bad)
        self.rands = S.random_multipliers(N_SETS, random.Random(0x61AB))


class DevPartial:
    """tbls_dev_batch_partial (or _idx with `idx`) + tbls_dev_final_verify of W.good in device memory."""

    def __init__(self, W, idx=None):
        import torch

        from teku_amd import native

        self.torch, self.native = torch, native
        pk, ms, sg = W.good
        n = len(pk)
        self.dev = torch.device("cuda", 0)
        u8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(self.dev)  # noqa: E731
        self.bufs = dict(pks=u8(b"".join(pk)), msgs=u8(b"".join(ms)), sigs=u8(b"".join(sg)),
                         pk_off=torch.arange(0, n + 1, dtype=torch.int32, device=self.dev),
                         msg_off=torch.arange(0, 32 * (n + 1), 32, dtype=torch.int32, device=self.dev),
                         rand=torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in W.rands], dtype=torch.int64, device=self.dev))
        self.idx = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=self.dev)
        b = self.bufs
        self.desc = native.TblsDevBatch(b["pks"].data_ptr(), b["pk_off"].data_ptr(), n, b["msgs"].data_ptr(), b["msg_off"].data_ptr(),
                                        b["sigs"].data_ptr(), b["rand"].data_ptr(), n)

    def __call__(self):
        """(the 580-byte record as hex, the final verification's verdict)"""
        torch, native = self.torch, self.native
        L = native.lib()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        out = torch.zeros(native.PARTIAL_BYTES, dtype=torch.uint8, device=self.dev)
        if self.idx is None:
            native.check(L.tbls_dev_batch_partial(0, ctypes.byref(self.desc), stream, out.data_ptr()), "partial")
        else:
            native.check(L.tbls_dev_batch_partial_idx(0, ctypes.byref(self.desc), self.idx.data_ptr(), stream, out.data_ptr()), "partial_idx")
        ok = ctypes.c_int(7)
        native.check(L.tbls_dev_final_verify(0, out.data_ptr(), 1, stream, ctypes.byref(ok)), "final")
        torch.cuda.synchronize()
        return bytes(out.cpu().numpy()).hex(), ok.value


def comb_stats():
    """[sets served, cache rows built, table rows built, capacity], the counters reset after reading."""
    from teku_amd import bls

    return list(bls.pk_comb_stats(reset=True))


def library_steps(W):
    """Every step of the library-level check, in order, each with the comb
    counters (reset) after it."""
    from teku_amd import bls

    out = {}

    def step(name, **kv):
        kv["comb"] = comb_stats()
        out[name] = kv

    bls.pk_cache_clear()
    comb_stats()
    part = DevPartial(W)
    for name in ("cold", "warm"):
        rec, ok = part()
        step(name, rec=rec, ok=ok)
    pk, ms, sg = W.bad
    arr = W.S.SetArray(b"".join(pk), [1] * N_SETS, b"".join(ms), [32] * N_SETS, b"".join(sg))
    ok, each = arr.batch_verify_each(W.rands)
    step("each_warm", ok=ok, each=each)
    bls.pk_cache_clear()
    ok, each = arr.batch_verify_each(W.rands)
    step("each_cold", ok=ok, each=each)
    bls.pk_cache_clear()
    for name in ("cleared_cold", "cleared_warm"):
        rec, ok = part()
        step(name, rec=rec, ok=ok)
    table = bls.ValidatorKeyTable(W.pk)
    step("table_load")
    by_idx = DevPartial(W, idx=[p % N_DISTINCT for p in range(N_SETS)])
    rec, ok = by_idx()
    step("by_index", rec=rec, ok=ok)
    rec, ok = part()  # byte keys that the table's index resolves: the table's rows
    step("bytes_with_table", rec=rec, ok=ok)
    table.clear()
    return out


def main():
    import torch  # noqa: F401  (one HIP runtime: torch's, teku_amd/native.py)

    from teku_amd import native

    native.lib()
    out = library_steps(World())
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
