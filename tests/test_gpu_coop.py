"""GPU parity of the lane-cooperative row arithmetic at its edges: the vectors
and Python-integer checks of tests/coop_cases.py (the ones tests/test_coop.py
runs on the host emulation) through the DPP code of tb_coop.h, tb_cinv.h and
tb_cpoint.h, via the raw-digit / raw-limb kernels of tests/native/k_test_coop.hip.
"""

import pytest

from oracle import bls12_381 as O
from tests import coop_cases as C
from tests.opcodec import dec_fp12, enc_fp, enc_fp2, enc_fp12, load_test_lib, run_ops

pytestmark = pytest.mark.gpu

P = C.P


@pytest.fixture(scope="module")
def run():
    L = load_test_lib()
    return lambda op, recs: run_ops(L.tbls_test_ops, op, recs)


def _i32(d):
    return b"".join(int(x).to_bytes(4, "little", signed=True) for x in d)


def _i64(d):
    return b"".join(int(x).to_bytes(8, "little", signed=True) for x in d)


def _digits(o):
    return [int.from_bytes(o[4 * j : 4 * j + 4], "little", signed=True) for j in range(16)]


def _be(v):
    return int(v).to_bytes(48, "big")


def _raw(o, off=0):
    return int.from_bytes(o[off : off + 48], "big")


def _mul_digits(run, A, B):
    return [_digits(o) for o in run("COOP_MUL_DIGITS", [_i32(a) + _i32(b) for a, b in zip(A, B)])]


# ---- product ----------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", C.MUL_CLASS_PAIRS)
def test_coop_mul_classes(run, ta, tb):
    """cmul at the class bounds of tb_coop.h (T_a T_b <= 7, worst-case digits of
    both signs), four different records per wave; digit for digit what the
    host emulation gives (the committed digest)."""
    A, B = C.mul_class_cases(ta, tb)
    out = _mul_digits(run, A, B)
    C.check_mul(A, B, out)
    assert C.digest(out) == C.golden_mul()["classes"]["%dx%d" % (ta, tb)]


def test_coop_mul_chain(run):
    outs = C.mul_chain(lambda A, B: _mul_digits(run, A, B))
    assert C.digest(*outs) == C.golden_mul()["chain"]


# ---- conversions ------------------------------------------------------------
def test_coop_fp_roundtrip(run):
    """cfrom_words / cmul / cdigits_to_fp on raw operands up to 2p - 1."""
    A, B = C.words_roundtrip_cases()
    out = run("COOP_MUL_WORDS", [_be(a) + _be(b) for a, b in zip(A, B)])
    C.check_mul_words(A, B, [_raw(o) for o in out])


def test_coop_to_fp_signed(run):
    D = C.to_fp_signed_cases()
    C.check_to_fp(D, [_raw(o) for o in run("COOP_TO_FP", [_i32(d) for d in D])])


def test_coop_to_fp_zero_residues(run):
    """Exactly 0 for every k p, |k| <= 64: what keeps the raw value p away from
    the row inversion (tb_cinv.h's contract)."""
    D = C.zero_residue_cases()
    C.check_zero_residues(D, [_raw(o) for o in run("COOP_TO_FP", [_i32(d) for d in D])])


# ---- creduce64 --------------------------------------------------------------
def test_coop_reduce(run):
    """The device branch of creduce64 (float estimate, bcast, mulw) against its
    contract.  No digest: host and device may round a tie differently."""
    X = C.reduce_cases()
    C.check_reduce(X, [_digits(o) for o in run("COOP_REDUCE", [_i64(x) for x in X])])


# ---- row inversion ----------------------------------------------------------
def test_coop_inv_raw_and_uniform(run):
    """inv_row_lane0 on raw limbs over [0, 2p) without p: the four-rows-per-wave
    form against A^-1 R^2, and the wave-uniform form with the early exit (one
    active row behind a branch, as the product calls it) limb for limb the
    same at every row position.  A = 1 must take strictly fewer cycles than a
    random A at every position: a build whose exit never fires shows."""
    A = C.inv_cases()
    raw = [_raw(o) for o in run("COOP_INV_RAW", [_be(a) for a in A])]
    C.check_inv(A, raw)
    # record i runs on row i & 3: every input once, the edge values on all four rows
    E = C.inv_edge_cases()
    U = A + [a for a in E for _ in range(4)]
    assert len(A) % 4 == 0
    exp = raw + [raw[A.index(a)] for a in E for _ in range(4)]
    out = run("COOP_INV_U", [_be(a) for a in U])
    assert [_raw(o) for o in out] == exp
    rnd = A[0]
    assert rnd.bit_length() > 370
    T = [1, 1, 1, 1, rnd, rnd, rnd, rnd]
    out = run("COOP_INV_U", [_be(a) for a in T])
    assert [_raw(o) for o in out] == [raw[A.index(a)] for a in T]
    cyc = [int.from_bytes(o[48:56], "little") for o in out]
    print("\nrow inversion with the early exit, cycles on rows 0..3: A = 1 %s, random A %s" % (cyc[:4], cyc[4:]))
    for one, r in zip(cyc[:4], cyc[4:]):
        assert one < r


# ---- row point arithmetic ---------------------------------------------------
def _points(run, group, op, k, A, B):
    tail = int(op).to_bytes(4, "little") + bytes(4) + int(k).to_bytes(8, "little")
    if group == 1:
        recs = [(enc_fp(a[0]) + enc_fp(a[1]) + enc_fp(b[0]) + enc_fp(b[1])).ljust(384, b"\0") + tail for a, b in zip(A, B)]
        out = run("COOP_POINT_G1", recs)
        return [tuple(_raw(o, 48 * j) * C.RINV % P for j in range(3)) for o in out]
    recs = [enc_fp2(a[0]) + enc_fp2(a[1]) + enc_fp2(b[0]) + enc_fp2(b[1]) + tail for a, b in zip(A, B)]
    out = run("COOP_POINT_G2", recs)
    res = []
    for o in out:
        c = [_raw(o, 48 * j) * C.RINV % P for j in range(6)]
        res.append(((c[0], c[1]), (c[2], c[3]), (c[4], c[5])))
    return res


@pytest.mark.parametrize("op", C.G1_OPS)
def test_cpoint_g1(run, op):
    A, B, k = C.point_cases(1, op)
    C.check_points(1, op, A, B, k, _points(run, 1, op, k, A, B))


@pytest.mark.parametrize("op", C.G2_OPS)
def test_cpoint_g2(run, op):
    A, B, k = C.point_cases(2, op)
    C.check_points(2, op, A, B, k, _points(run, 2, op, k, A, B))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("op", C.EXCEPTIONAL_OPS)
def test_cpoint_exceptional(run, group, op):
    A, B = C.exceptional_cases(group)
    C.check_exceptional(group, op, _points(run, group, op, 0, A, B))


# ---- coop Fp12 inversion and final exponentiation at 0 and 1 ----------------
def test_cfe_inv_and_final_exp_at_zero_and_one(run):
    """The value-dependent early exit of the row inversion inside the coop Fp12
    inversion: f = 0 and f = 1 equal the single-lane kernels bit for bit."""
    z2 = (0, 0)
    zero = ((z2, z2, z2), (z2, z2, z2))
    one = (((1, 0), z2, z2), (z2, z2, z2))
    fs = [zero, one]
    op5 = (5).to_bytes(4, "little")
    inv = run("CFE_OPS", [enc_fp12(f) + enc_fp12(one) + op5 for f in fs])
    assert [x[:576] for x in inv] == [x[:576] for x in run("FP12_INV", [enc_fp12(f) for f in fs])]
    assert [dec_fp12(x) for x in inv] == [zero, one]
    fe = run("FINAL_EXP_COOP", [enc_fp12(f) for f in fs])
    assert [x[:576] for x in fe] == [x[:576] for x in run("FINAL_EXP", [enc_fp12(f) for f in fs])]
    assert dec_fp12(fe[1]) == one
    assert O.final_exponentiation(one) == one
