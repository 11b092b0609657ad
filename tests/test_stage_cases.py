"""The shared stage cases (tests/stage_cases.py) and their reference, checked
against themselves without a GPU: the reference adds and multiplies decoded
points, the identities here go through the secret keys instead, and every edge
tests/test_gpu_stages.py relies on is present in the case lists."""

import pytest

from oracle import bls12_381 as O
from tests import stage_cases as S


@pytest.fixture(scope="module")
def key_sets():
    return S.key_sets()


@pytest.fixture(scope="module")
def msm():
    cases = S.msm_cases()
    return cases, [S.msm_reference(c) for c in cases]


def test_decoders_invert_the_montgomery_form():
    x = 0x1234567890ABCDEF
    limbs = (x << 406) % S.P
    assert S.dec_fp(limbs.to_bytes(48, "little")) == x
    assert S.dec_g1(bytes(96)) == S.ZERO_G1 and S.dec_g2(bytes(192)) == S.ZERO_G2


def test_edge_randomizers_are_all_there():
    er = S.edge_rands()
    assert len(er) == len(set(er)) and all(1 <= r < 1 << 64 for r in er)
    assert set([1, 2, 3, 4, 5, 7, 1 << 63, S.M64, 0x8000000000000001, 0x5555555555555555, 0xC000000000000003, 0x100000000]) <= set(er)
    assert {d << (8 * w) for d in (1, 255) for w in range(8)} <= set(er)
    assert {0xFF, 0x100, 0x101, 0x00FF00FF00FF00FF, 0xFF00FF00FF00FF00, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x0100000000000001} <= set(er)
    # mul_u64_aff_w2's first window: digit 1 at an even top bit, 2 and 3 at an odd one
    tops = {((r.bit_length() - 1) & 1, r >> (2 * ((r.bit_length() - 1) >> 1))) for r in er}
    assert {(0, 1), (1, 2), (1, 3)} <= tops
    assert any(r.bit_length() == 63 for r in er) and any(r.bit_length() == 64 for r in er)
    # every 2-bit digit occurs below the top window too (the table's three entries and the skipped zero)
    assert {(r >> (2 * w)) & 3 for r in er for w in range((r.bit_length() - 1) >> 1)} == {0, 1, 2, 3}
    assert len(S.seeded_rands(41, 36)) == 36 and 0 not in S.seeded_rands(41, 36)


def test_key_cases_cover_the_edges(key_sets):
    n = len(key_sets)
    assert n <= 130 and n % 4 and n % 64 and n > 64  # k_keys_coop's rows, a partial last block, two blocks
    singles = [s for s in key_sets if len(s.keys) == 1 and s.sks[0] is not None]
    assert set(S.edge_rands()) <= {s.r for s in singles}
    assert sum(1 for s in singles if s.tag == "random r") >= 24
    tags = [s.tag for s in key_sets]
    for t in S.INVALID_KEYS + tuple(f"multi {k}" for k in S.MULTI_SIZES) + ("P, P", "P, -P", "P, -P, Q", "multi with an invalid member"):
        assert tags.count(t) == 1, t
    assert all(1 <= s.r < 1 << 64 for s in key_sets)
    by = {s.tag: s for s in key_sets}
    assert [len(by[f"multi {k}"].keys) for k in S.MULTI_SIZES] == list(S.MULTI_SIZES)
    assert by["P, P"].keys[0] == by["P, P"].keys[1]
    assert sum(by["P, -P"].sks) % O.R == 0 and sum(by["P, -P, Q"].sks) % O.R != 0
    assert sum(1 for k in by["multi with an invalid member"].sks if k is None) == 1
    # the invalid keys fail for the reasons their tags give
    want = {"infinity key": O.PK_IS_INFINITY, "bad encoding": O.BAD_ENCODING, "off-curve x": O.POINT_NOT_ON_CURVE, "outside G1": O.POINT_NOT_IN_GROUP}
    for t, code in want.items():
        assert O.pk_decode_validate(by[t].keys[0])[0] == code, t
    assert O.on_curve_g1(O.g1_decompress(by["outside G1"].keys[0])[1])


def test_key_reference_identities(key_sets):
    """[r] sum pk(sk_j) == pk(r sum sk_j mod R), and P2 == -pk(r); codes as stage_set_pk."""
    batch = S.key_batch(key_sets)
    ref = S.key_reference(batch)
    unit = S.key_reference(batch, unit_r=True)
    for s, (p, p2, code), (pu, p2u, cu) in zip(key_sets, ref, unit):
        x, y = S.g1_of_bytes(S.pk_of(s.r))
        assert p2 == (x, (-y) % S.P) == p2u, s.tag
        total = None if None in s.sks else sum(s.sks) % O.R
        if not total:
            assert (p, code) == (S.ZERO_G1, O.PK_IS_INFINITY) == (pu, cu), s.tag
        else:
            assert (p, code) == (S.g1_of_bytes(S.pk_of(s.r * total)), O.SUCCESS), s.tag
            assert (pu, cu) == (S.g1_of_bytes(S.pk_of(total)), O.SUCCESS), s.tag
    assert sum(1 for _, _, c in ref if c) == len(S.INVALID_KEYS) + 2


def test_key_table_form(key_sets):
    """The table form addresses the same keys: the same reference, plus the
    two sets with an index past the table (BAD_ENCODING, no point)."""
    byte, tab = S.key_batch(key_sets), S.key_batch_table(key_sets)
    assert tab.n_keys == tab.tab_n == byte.n_keys and len(tab.rands) == len(byte.rands) + 2
    assert tab.key_idx[: byte.n_keys] != list(range(byte.n_keys))  # not the identity
    ref_b, ref_t = S.key_reference(byte), S.key_reference(tab)
    assert ref_t[: len(ref_b)] == ref_b
    assert [(p, c) for p, _, c in ref_t[len(ref_b) :]] == [(S.ZERO_G1, O.BAD_ENCODING)] * 2
    past = [tab.key_idx[tab.pk_off[i] : tab.pk_off[i + 1]] for i in (len(ref_b), len(ref_b) + 1)]
    assert past[0] == [tab.tab_n] and len(past[1]) == 3 and sum(k >= tab.tab_n for k in past[1]) == 1


def test_sig_check_cases_cover_the_edges():
    sigs = S.check_sigs()
    n = len(sigs)
    assert n % 4 and n % 64 and n > 64
    ref = S.sig_reference(sigs)
    codes = [c for _, _, c in ref]
    assert {O.SUCCESS, O.BAD_ENCODING, O.POINT_NOT_ON_CURVE, O.POINT_NOT_IN_GROUP} == set(codes)
    assert codes.count(O.BAD_ENCODING) == 3 and codes[n - 1] == O.POINT_NOT_IN_GROUP
    inf = [i for i, b in enumerate(sigs) if b == O.INFINITY_G2]
    assert len(inf) == 2 and all(ref[i] == (S.ZERO_G2, 1, O.SUCCESS) for i in inf)
    assert {i % 4 for i, c in enumerate(codes) if c} == {0, 1, 2, 3}  # every row of a workgroup
    for q, skip, code in ref:
        assert (skip == 0) == (code == O.SUCCESS and q != S.ZERO_G2)
        assert skip or (O.on_curve_g2(q) and O.g2_in_group_slow(O.jac_from_affine(O.FP2, q)))


def test_msm_cases_cover_the_edges(msm):
    cases, refs = msm
    by = {c.name: (c, r) for c, r in zip(cases, refs)}
    assert len(by) == len(cases)
    assert all(1 <= r < 1 << 64 for c in cases for r in c.rands)
    assert (len(by["one set, r = 1"][0].sigs), by["one set, r = 1"][0].rands) == (1, [1])
    assert by["33 sets, r = 2^64 - 1"][0].rands == [S.M64] * 33
    for n in S.SHARED_DIGIT_SIZES:  # one bucket of exactly n entries
        c = by[f"{n} sets share a byte-0 digit"][0]
        assert len(c.sigs) == n and {r & 0xFF for r in c.rands} == {0x5A}
        assert n < 2 or len(set(c.rands)) > 1
    assert set(S.SHARED_DIGIT_SIZES) == {1, 31, 32, 33, 64, 65}
    for n in S.REPEAT_SIZES:
        c = by[f"one signature {n} times, one r"][0]
        assert len(c.sigs) == n and len(set(c.sigs)) == 1 and len(set(c.rands)) == 1
    assert set(S.REPEAT_SIZES) == {2, 3, 32, 64}
    # A, -A in one bucket: every pair skipped
    c, (pairs, codes, n_bad, total) = by["A, -A, one r"]
    assert sum(c.sks) % O.R == 0 and all(p[1:] == (S.ZERO_G2, 1) for p in pairs) and (n_bad, total) == (0, 2)
    c, (pairs, _, _, _) = by["A, -A, B, one r"]
    assert [p[2] for p in pairs[:8]] == [0, 0, 1, 1, 1, 1, 0, 0]
    assert {p[1] for p in pairs if not p[2]} == {S.g2_of_bytes(c.sigs[2])}
    # A and -A in two buckets (digits 1 and 3) of bit-sum 0: cancelled by the tree, and -A alone in bit-sum 1
    c, (pairs, _, _, _) = by["A r = 1, -A r = 3"]
    assert c.rands == [1, 3] and pairs[0][1:] == (S.ZERO_G2, 1) and pairs[1][1:] == (S.g2_of_bytes(c.sigs[1]), 0)
    c, (pairs, codes, n_bad, total) = by["infinite and invalid signatures in used buckets"]
    assert c.sigs.count(O.INFINITY_G2) == 1 and n_bad == 1 and sorted(codes) == [0] * 5 + [O.POINT_NOT_IN_GROUP]
    assert len(set(c.rands)) == 1 and total == 2 * len(c.sigs)  # they are counted and scattered, then left out
    c = by["edge randomizers (zero bytes)"][0]
    assert set(c.rands) == set(S.edge_rands()) and any((r >> (8 * w)) & 0xFF == 0 for r in c.rands for w in range(8))
    assert len(by["300 sets, seeded r"][0].sigs) == 300
    # a finite V[w][k] in every case but the all-cancelling one, an infinite one in most
    for c, (pairs, _, _, _) in zip(cases, refs):
        assert c.name == "A, -A, one r" or any(not p[2] for p in pairs), c.name
    assert sum(1 for _, (pairs, _, _, _) in zip(cases, refs) if any(p[2] for p in pairs)) >= 12


def test_msm_reference_identity(msm):
    """sum_j [2^j] V_j == sum_i [r_i] sig_i == [sum_i r_i sk_i] H(MSG), and
    P_j == -pk(2^j); the bucket view sums to the same pairs."""
    cases, refs = msm
    g = S.neg_pow2_g1()
    for j in (0, 1, 7, 8, 63):
        x, y = S.g1_of_bytes(S.pk_of(1 << j))
        assert g[j] == (x, (-y) % S.P)
    for c, (pairs, codes, n_bad, total) in zip(cases, refs):
        assert [p[0] for p in pairs] == g
        acc = O.jac_inf(O.FP2)
        for j in reversed(range(64)):
            acc = O.jac_double(O.FP2, acc)
            if not pairs[j][2]:
                acc = O.jac_add(O.FP2, acc, O.jac_from_affine(O.FP2, pairs[j][1]))
        k = sum(r * sk for r, sk in zip(c.rands, c.sks) if sk is not None) % O.R
        want = S.g2_of_bytes(S.sig_of(k)) if k else None
        assert O.jac_to_affine(O.FP2, acc) == want, c.name
        assert n_bad == sum(1 for x in codes if x)
    for c, (pairs, _, _, _) in list(zip(cases, refs))[:-1]:  # the bucket view, all but the largest case
        b = S.bucket_reference(c)
        for j in range(64):
            acc = O.jac_inf(O.FP2)
            for (w, d), a in b.items():
                if w == j // 8 and (d >> (j % 8)) & 1:
                    acc = O.jac_add(O.FP2, acc, O.jac_from_affine(O.FP2, a))
            assert (O.jac_to_affine(O.FP2, acc) or S.ZERO_G2) == pairs[j][1], (c.name, j)


def test_hash_rand_reference_identity():
    """[r] H(m) is the signature of m by the secret key r."""
    from oracle import c_oracle as C

    msgs, rands = S.hash_rand_cases()
    assert set(S.edge_rands()) <= set(rands) and 1 in rands and {0, 768} <= {len(m) for m in msgs}
    ref = S.hash_rand_reference(msgs, rands)
    for m, r, q in zip(msgs, rands, ref):
        assert q == S.g2_of_bytes(C.sign(r, m)), hex(r)
