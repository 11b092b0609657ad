"""Byte-level parity of the key and signature stage kernels of a randomized
batch, and of the hash kernel's randomizer branch.

Before the Miller loop a batch runs three device stages.  The hash stage is
compared at its own output in tests/test_gpu_hash_variants.py; this module
does the same for the other two.  Through the test library's hook
(tests/native/k_test_stages.hip), which launches the PRODUCT library's kernels
with the grids and blocks of tb_lib.hip, every form of the key stage
(k_set_pk, k_set_pk_w2 and its LDS window table, k_keys_coop, k_set_pk_wave,
k_set_pk_agg_coop; keys as bytes and from a table; the r = 1 forms), the three
signature checks (k_sig_check, k_sig_check_w2, k_sig_check_coop), the
bucket-sum chain (k_msm_hist, k_msm_scan, k_msm_scatter, k_msm_bucket_tree,
k_msm_bitsum_pairs) and k_set_hash_coop with a randomizer run on the cases of
tests/stage_cases.py -- edge randomizers, cancelling and repeated points,
bucket lengths around the 32-lane chunking, invalid and infinite inputs -- at
sizes of a few hundred sets, far below the product's thresholds for these
kernels (20,480 and 32,768 sets).  Points, flags, codes and n_bad must equal
the plain reference exactly; there is no tolerance.  A failing bucket-sum pair
is reported with the buckets that differ.  tests/test_stage_cases.py checks
the same reference against itself without a GPU.
"""

import ctypes

import pytest

from oracle import bls12_381 as O
from oracle import c_oracle as C
from oracle.keys import interop_sk
from tests import stage_cases as S

pytestmark = pytest.mark.gpu

KEY_VARIANTS = {0: "k_set_pk", 1: "k_set_pk_w2", 2: "k_keys_coop", 3: "k_set_pk + k_set_pk_wave", 4: "k_set_pk + k_set_pk_agg_coop"}
KEY_UNIT_VARIANTS = (0, 1, 4)
SIG_VARIANTS = {0: "k_sig_check", 1: "k_sig_check_w2", 2: "k_sig_check_coop"}
MSM_VARIANTS = {3: "chain with k_sig_check", 4: "chain with k_sig_check_w2"}
UNWRITTEN = b"\xee" * 48


def _launched(rc, what):
    """A hook's negative code is a failed HIP call (a launch, a copy, the
    synchronize): nothing more may run on that device, so the session ends."""
    if rc:
        pytest.exit(f"tests/native/k_test_stages.hip: {what}: HIP call failed ({rc}); no further GPU work", returncode=3)


@pytest.fixture(scope="module")
def hook():
    from teku_amd import native
    from tests.opcodec import load_test_lib

    L = load_test_lib()
    vp, cp, sz, ci, u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    L.tbls_test_key_stage.restype = ci
    L.tbls_test_key_stage.argtypes = [cp, ci, cp, sz, vp, vp, u32, vp, sz, ci, vp, vp, vp, vp]
    L.tbls_test_sig_stage.restype = ci
    L.tbls_test_sig_stage.argtypes = [cp, ci, cp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.tbls_test_hash_rand.restype = ci
    L.tbls_test_hash_rand.argtypes = [cp, cp, vp, sz, cp, sz, vp, vp, vp]
    so = native.LIB_PATH.encode()

    def u32s(v):
        return (ctypes.c_uint32 * len(v))(*v)

    def u64s(v):
        return (ctypes.c_uint64 * len(v))(*v)

    class Hook:
        @staticmethod
        def keys(variant, b, unit_r=False):
            """[(P, P2, code)] per set, n_bad."""
            n = len(b.rands)
            p, p2, code = (ctypes.create_string_buffer(k * n) for k in (96, 96, 1))
            bad = ctypes.c_uint32(0xEEEEEEEE)
            idx = u32s(b.key_idx) if b.key_idx is not None else None
            rc = L.tbls_test_key_stage(so, variant, b.blob, b.n_keys, u32s(b.pk_off), idx, b.tab_n, u64s(b.rands), n, int(unit_r), p, p2, code,
                                       ctypes.byref(bad))
            _launched(rc, KEY_VARIANTS[variant])
            for name, buf in (("P", p.raw), ("P2", p2.raw)):
                blank = [i for i in range(n) if UNWRITTEN in buf[96 * i : 96 * i + 96]]
                assert not blank, (KEY_VARIANTS[variant], name, "not written", blank[:8], [b.tags[i] for i in blank[:8]])
            return [(S.dec_g1(p.raw[96 * i : 96 * i + 96]), S.dec_g1(p2.raw[96 * i : 96 * i + 96]), code.raw[i]) for i in range(n)], bad.value

        @staticmethod
        def sigs(variant, sigs):
            """[(Q, skip, code)] per signature, n_bad."""
            n = len(sigs)
            q, flag, code = (ctypes.create_string_buffer(k * n) for k in (192, 1, 1))
            bad = ctypes.c_uint32(0xEEEEEEEE)
            rc = L.tbls_test_sig_stage(so, variant, b"".join(sigs), None, n, q, flag, code, ctypes.byref(bad), None, None, None)
            _launched(rc, SIG_VARIANTS[variant])
            return [(S.dec_g2(q.raw[192 * i : 192 * i + 192]), flag.raw[i], code.raw[i]) for i in range(n)], bad.value

        @staticmethod
        def msm(variant, case):
            """(pairs [(P_j, Q_j, skip_j)], codes, n_bad, off[2048], raw bucket sums)."""
            n = len(case.sigs)
            q, flag, code, p = (ctypes.create_string_buffer(k) for k in (192 * 64, 64, n, 96 * 64))
            buckets = ctypes.create_string_buffer(2048 * 288)
            bad, total = ctypes.c_uint32(0xEEEEEEEE), ctypes.c_uint32(0xEEEEEEEE)
            rc = L.tbls_test_sig_stage(so, variant, b"".join(case.sigs), u64s(case.rands), n, q, flag, code, ctypes.byref(bad), p,
                                       ctypes.byref(total), buckets)
            _launched(rc, MSM_VARIANTS[variant] + ", " + case.name)
            pairs = [(S.dec_g1(p.raw[96 * j : 96 * j + 96]), S.dec_g2(q.raw[192 * j : 192 * j + 192]), flag.raw[j]) for j in range(64)]
            return pairs, list(code.raw), bad.value, total.value, buckets.raw

        @staticmethod
        def hash_rand(msgs, rands):
            n = len(msgs)
            off = [0]
            for m in msgs:
                off.append(off[-1] + len(m))
            q, skip = ctypes.create_string_buffer(192 * n), ctypes.create_string_buffer(n)
            rc = L.tbls_test_hash_rand(so, b"".join(msgs) or b"\0", u32s(off), n, O.ETH2_DST, len(O.ETH2_DST), u64s(rands), q, skip)
            _launched(rc, "k_set_hash_coop with rand")
            return [None if skip.raw[i] else S.dec_g2(q.raw[192 * i : 192 * i + 192]) for i in range(n)], list(skip.raw)

    return Hook


# ---- key stage -----------------------------------------------------------------
@pytest.fixture(scope="module")
def key_cases():
    sets = S.key_sets()
    byte, tab = S.key_batch(sets), S.key_batch_table(sets)
    return {"bytes": (byte, S.key_reference(byte)), "table": (tab, S.key_reference(tab)), "bytes r=1": (byte, S.key_reference(byte, unit_r=True)),
            "table r=1": (tab, S.key_reference(tab, unit_r=True))}


def _assert_keys(name, batch, got, n_bad, want):
    for i, (g, w) in enumerate(zip(got, want)):
        for what, a, b in zip(("P", "P2", "set_code"), g, w):
            assert a == b, (name, "set", i, batch.tags[i], "r", hex(batch.rands[i]), what)
    assert n_bad == sum(1 for _, _, c in want if c), name


@pytest.mark.parametrize("variant", sorted(KEY_VARIANTS), ids=[KEY_VARIANTS[v] for v in sorted(KEY_VARIANTS)])
def test_key_stage_bytes(hook, key_cases, variant):
    """P = [r] apk, P2 = -[r] g1, set_code and n_bad of every form on byte keys."""
    batch, want = key_cases["bytes"]
    got, n_bad = hook.keys(variant, batch)
    _assert_keys(KEY_VARIANTS[variant], batch, got, n_bad, want)


@pytest.mark.parametrize("variant", sorted(KEY_VARIANTS), ids=[KEY_VARIANTS[v] for v in sorted(KEY_VARIANTS)])
def test_key_stage_table(hook, key_cases, variant):
    """The same keys from a table through key_idx / tab_n (k_keys_coop with
    pks null), with two sets indexing past the table."""
    batch, want = key_cases["table"]
    got, n_bad = hook.keys(variant, batch)
    _assert_keys(KEY_VARIANTS[variant] + " (table)", batch, got, n_bad, want)


@pytest.mark.parametrize("form", ["bytes", "table"])
@pytest.mark.parametrize("variant", KEY_UNIT_VARIANTS, ids=[KEY_VARIANTS[v] for v in KEY_UNIT_VARIANTS])
def test_key_stage_unit_r(hook, key_cases, variant, form):
    """multi_wave & 4 / unit_r = 1: P = apk unmultiplied, P2 = -[r] g1 still."""
    batch, want = key_cases[form + " r=1"]
    got, n_bad = hook.keys(variant, batch, unit_r=True)
    _assert_keys(KEY_VARIANTS[variant] + " (r = 1, " + form + ")", batch, got, n_bad, want)


def test_key_stage_forms_agree(hook, key_cases):
    """Every form returns what the others return, byte keys and table alike."""
    for form, variants in (("bytes", KEY_VARIANTS), ("table", KEY_VARIANTS), ("bytes r=1", KEY_UNIT_VARIANTS), ("table r=1", KEY_UNIT_VARIANTS)):
        batch = key_cases[form][0]
        outs = {v: hook.keys(v, batch, unit_r=form.endswith("r=1")) for v in variants}
        first = outs[min(outs)]
        for v, o in outs.items():
            assert o == first, (form, KEY_VARIANTS[v])
    n = len(key_cases["bytes"][0].rands)
    assert hook.keys(0, key_cases["table"][0])[0][:n] == hook.keys(0, key_cases["bytes"][0])[0]


# ---- signature checks ------------------------------------------------------------
@pytest.fixture(scope="module")
def sig_cases():
    sigs = S.check_sigs()
    return sigs, S.sig_reference(sigs)


@pytest.mark.parametrize("variant", sorted(SIG_VARIANTS), ids=[SIG_VARIANTS[v] for v in sorted(SIG_VARIANTS)])
def test_sig_check(hook, sig_cases, variant):
    """Q, the skip flag, sig_code and n_bad of the three checks (skip mode 1)."""
    sigs, want = sig_cases
    got, n_bad = hook.sigs(variant, sigs)
    for i, (g, w) in enumerate(zip(got, want)):
        for what, a, b in zip(("Q", "skip", "sig_code"), g, w):
            assert a == b, (SIG_VARIANTS[variant], "signature", i, what)
    assert n_bad == sum(1 for _, _, c in want if c)


def test_sig_checks_agree(hook, sig_cases):
    outs = [hook.sigs(v, sig_cases[0]) for v in sorted(SIG_VARIANTS)]
    assert outs[0] == outs[1] == outs[2]


# ---- bucket sums -----------------------------------------------------------------
@pytest.fixture(scope="module")
def msm_cases():
    cases = S.msm_cases()
    return cases, [S.msm_reference(c) for c in cases]


def _wrong_buckets(case, raw):
    """The buckets (window, digit) whose device sum differs from the reference's."""
    out = []
    for (w, d), want in sorted(S.bucket_reference(case).items()):
        b = 256 * w + d
        if S.dec_g2j(raw[288 * b : 288 * b + 288]) != want:
            out.append((w, d))
    return out


@pytest.mark.parametrize("variant", sorted(MSM_VARIANTS), ids=[MSM_VARIANTS[v] for v in sorted(MSM_VARIANTS)])
def test_bucket_sum_chain(hook, msm_cases, variant):
    """The chain as sig_chain queues it: the 64 pairs (-[2^j] g1, V_j, skip_j),
    sig_code, n_bad and the scan's total, case by case."""
    for case, (pairs, codes, n_bad, total) in zip(*msm_cases):
        g_pairs, g_codes, g_bad, g_total, raw = hook.msm(variant, case)
        assert g_total == total, (case.name, "off[2048]")
        assert g_codes == codes and g_bad == n_bad, (case.name, "sig_code / n_bad")
        for j, (g, w) in enumerate(zip(g_pairs, pairs)):
            if g != w:
                what = [k for k, a, b in zip(("P", "Q", "skip"), g, w) if a != b]
                pytest.fail(f"{MSM_VARIANTS[variant]}, {case.name}: pair {j} (window {j // 8}, bit {j % 8}) differs in {what}; "
                            f"wrong buckets (window, digit): {_wrong_buckets(case, raw)}")


def test_bucket_sum_chains_agree(hook, msm_cases):
    for case in msm_cases[0]:
        a, b = hook.msm(3, case), hook.msm(4, case)
        assert a[:4] == b[:4], case.name


# ---- hash with a randomizer --------------------------------------------------------
def test_hash_with_randomizer(hook):
    """k_set_hash_coop with rand non-null: Q = [r] H(m) (r = 1: H(m) itself)."""
    msgs, rands = S.hash_rand_cases()
    want = S.hash_rand_reference(msgs, rands)
    got, skip = hook.hash_rand(msgs, rands)
    assert skip == [0] * len(msgs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, ("set", i, "r", hex(rands[i]), "message bytes", len(msgs[i]))


# ---- the public API on the edge randomizers ------------------------------------------
@pytest.mark.parametrize("keys_per_set", [1, 2])
def test_batch_verify_edge_randomizers(keys_per_set):
    """About 40 sets of one key, and of two keys (the multi-key plan), with
    every randomizer from the edge list: the valid batch verifies, the batch
    with two sets' signatures swapped does not, both as the C oracle says on
    the same randomizers."""
    import torch  # noqa: F401  (share torch's HIP runtime in-process)

    from teku_amd import bls

    rands = S.edge_rands()
    rands += S.seeded_rands(80, max(0, 40 - len(rands)))
    n = len(rands)
    assert rands[3] != rands[n - 1]  # equal randomizers would hide the swap below
    sks = [[interop_sk(5000 + keys_per_set * i + j) for j in range(keys_per_set)] for i in range(n)]
    msgs = [i.to_bytes(2, "big") * 16 for i in range(n)]
    pks = [[C.sk_to_pk(s) for s in ss] for ss in sks]
    sigs = [C.sign(sum(ss) % O.R, m) for ss, m in zip(sks, msgs)]
    swapped = list(sigs)
    swapped[3], swapped[n - 1] = swapped[n - 1], swapped[3]
    for sg, want in ((sigs, True), (swapped, False)):
        got = bls.batch_verify_raw([(b"".join(p), len(p), m, s) for p, m, s in zip(pks, msgs, sg)], rands)
        assert got is want
        assert C.batch_verify_sets(pks, msgs, sg, rands) is want
