"""The KZG point and term kernels in both of their forms, launched directly
(tests/native/k_test_kzg.hip looks the product library's own kernels up by
name): k_kzg_points / k_kzg_points_coop and k_kzg_terms / k_kzg_terms_coop.

The host API sends every batch of at most 1,024 blobs to the lane-cooperative
forms, so the suite's batches never reach the one-lane k_kzg_terms through it,
and k_kzg_points only decodes one valid commitment (compute_blob_kzg_proof).
Here both forms get the same inputs (tests/kzg_cases.py) and must agree with
each other and with the Python oracle, bit for bit:
  terms   every T[k] of the documented term list, for z over the edge scalars
          of the GLV split (multiples of mu, 0, r - 1, ...), chosen r and y,
          infinity flags on commitments and proofs;
  points  code, infinity flag and the affine point, for valid encodings and
          every kind of encoding the kernels must reject, in each row of a
          4-row workgroup and with partly filled workgroups.
Every input is a well-formed byte string; nothing is out of range."""

import pytest

from tests import kzg_cases as C
from tests.opcodec import kzg_kernel_runner, load_test_lib

pytestmark = pytest.mark.gpu

FORMS = [(0, "one-lane"), (1, "coop")]


@pytest.fixture(scope="module")
def run():
    return kzg_kernel_runner(load_test_lib())


@pytest.fixture(scope="module")
def term_refs():
    cases = C.term_cases()
    return cases, [C.term_expected(c) for c in cases]


def test_term_cases_cover_the_edges():
    cases = C.term_cases()
    zs = {z for c in cases for z in c[4]}
    assert set(C.mul_scalars()) <= zs
    assert {c[0] for c in cases} == {1, 3}
    assert {1, C.R - 1, C.MU} <= {c[6] for c in cases if c[0] == 3}
    assert any(sum(c[3][: c[0]]) and sum(c[3][c[0] :]) for c in cases)  # a commitment and a proof at infinity
    assert any(sum(c[3][: c[0]]) and not sum(c[3][c[0] :]) for c in cases) and any(sum(c[3][c[0] :]) and not sum(c[3][: c[0]]) for c in cases)
    n, _, _, _, _, y, r = cases[-1]
    assert (n, r, y) == (3, 1, [1, C.R - 1, 0])  # sum r^i y_i = 0 from non-zero terms
    sums = {sum(pow(c[6] if c[0] > 1 else 1, i, C.R) * c[5][i] for i in range(c[0])) % C.R for c in cases}
    assert {0, C.R - 1, C.MU} <= sums


@pytest.mark.parametrize("coop,name", FORMS, ids=[f[1] for f in FORMS])
def test_terms_match_oracle(run, term_refs, coop, name):
    cases, refs = term_refs
    for case, want in zip(cases, refs):
        n = case[0]
        got = [C.dec_term(o) for o in run(1, coop, C.term_input(case), n, 3 * n + 1)]
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, "n", n, "term", k, "z", [hex(z) for z in case[4]], "r", hex(case[6]), "inf", case[3])


@pytest.mark.parametrize("coop,name", FORMS, ids=[f[1] for f in FORMS])
def test_points_match_oracle(run, coop, name):
    for label, batch in C.point_batches():
        out = run(0, coop, b"".join(batch), len(batch), len(batch))
        for i, (b, o) in enumerate(zip(batch, out)):
            code, inf, a = C.point_expected(b)
            assert (o[0], o[1]) == (code, inf), (name, label, "index", i, b.hex())
            if a is not None:
                assert C.dec_aff(o[4:100]) == a, (name, label, "index", i)


def test_point_cases_cover_the_edges():
    from oracle import bls12_381 as O

    codes = {n: C.point_expected(b)[0] for n, b in C.bad_points().items()}
    assert all(codes.values()), codes  # every bad input is rejected by the oracle
    assert {O.BAD_ENCODING, O.POINT_NOT_ON_CURVE, O.POINT_NOT_IN_GROUP} == set(codes.values())
    assert codes["x = 0"] == codes["x = 0, sign bit"] == O.POINT_NOT_IN_GROUP
    assert all(codes[f"order {m}"] == O.POINT_NOT_IN_GROUP for m in (3, 11, 33)) and codes["rand non-G1"] == O.POINT_NOT_IN_GROUP
    assert all(C.point_expected(b)[0] == 0 for b in C.good_points())
    assert {len(b) for _, b in C.point_batches()} == set(C.POINT_COUNTS)
