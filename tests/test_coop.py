"""Lane-cooperative Fp products (teku_amd/csrc/tb_coop.h) on the host emulation
of a 16-lane row, checked against Python integers.

The digit-class bounds of the file comment are exercised with worst-case
digits (every digit at its class bound, both signs), the conversions from and
to the 12 x 32-bit [0, 2p) form with edge values, and a chain of products fed
back as operands (what the serial exponentiations do).  Test infrastructure
only.  The vectors and checks live in tests/coop_cases.py; tests/test_gpu_coop.py
runs the same ones through the DPP code on the GPU.
"""

import ctypes
import random

import numpy as np
import pytest

from tests import coop_cases as C

P = C.P
R = C.R
RINV = C.RINV


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    L = ctypes.CDLL(ge.build_hostsim())
    for name in ("tbls_hostsim_coop_mul_digits", "tbls_hostsim_coop_mul_fp"):
        getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.tbls_hostsim_coop_to_fp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.tbls_hostsim_coop_reduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.tbls_hostsim_coop_inv_raw.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    for name in ("tbls_hostsim_cpoint_g1", "tbls_hostsim_cpoint_g2"):
        getattr(L, name).argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64]
    return L


def _words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def _unwords(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def _word_rows(vals):
    return np.ascontiguousarray(np.array([_words(v) for v in vals], dtype=np.uint32))


def mul_digits(L, A, B):
    a = np.ascontiguousarray(np.array(A, dtype=np.int32))
    b = np.ascontiguousarray(np.array(B, dtype=np.int32))
    out = np.zeros_like(a)
    L.tbls_hostsim_coop_mul_digits(a.ctypes.data, b.ctypes.data, out.ctypes.data, len(A))
    return out


@pytest.mark.parametrize("ta,tb", C.MUL_CLASS_PAIRS)
def test_coop_mul_classes(lib, ta, tb):
    """Random and worst-case digits of every class pair with T_a T_b <= 7; the
    digits also match the committed digest (what the GPU must reproduce)."""
    A, B = C.mul_class_cases(ta, tb)
    out = mul_digits(lib, A, B)
    C.check_mul(A, B, out)
    assert C.digest(out) == C.golden_mul()["classes"]["%dx%d" % (ta, tb)]


def test_coop_mul_chain(lib):
    """Outputs fed back as operands, and sums of up to 7 outputs times an output."""
    outs = C.mul_chain(lambda A, B: mul_digits(lib, A, B))
    assert C.digest(*outs) == C.golden_mul()["chain"]


def test_coop_fp_roundtrip(lib):
    """[0, 2p) 12-word operands through cfrom_words / cmul / cdigits_to_fp equal
    fp_mul's residue, with the result back in [0, 2p)."""
    A, B = C.words_roundtrip_cases()
    a, b = _word_rows(A), _word_rows(B)
    out = np.zeros_like(a)
    lib.tbls_hostsim_coop_mul_fp(a.ctypes.data, b.ctypes.data, out.ctypes.data, len(A))
    C.check_mul_words(A, B, [_unwords(r) for r in out])


def _to_fp(lib, D):
    d = np.ascontiguousarray(np.array(D, dtype=np.int32))
    out = np.zeros((len(D), 12), dtype=np.uint32)
    lib.tbls_hostsim_coop_to_fp(d.ctypes.data, out.ctypes.data, len(D))
    return [_unwords(r) for r in out]


def test_coop_to_fp_signed(lib):
    """cdigits_to_fp on signed digit vectors of |value| < 64p."""
    D = C.to_fp_signed_cases()
    C.check_to_fp(D, _to_fp(lib, D))


def test_coop_to_fp_zero_residues(lib):
    """cdigits_to_fp returns exactly 0 (never p) for every multiple of p in its
    range: the half of inv_row_lane0's contract its callers supply."""
    D = C.zero_residue_cases()
    C.check_zero_residues(D, _to_fp(lib, D))


def test_coop_pow_win(lib):
    """cpow_win_n<2> with the (p+1)/4 schedule equals a^((p+1)/4) (Montgomery
    form in and out: the residue a R^-1 ... handled by comparing x^2 == a)."""
    lib.tbls_hostsim_coop_sqrt_cand.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    rng = random.Random(9)
    vals = [rng.randrange(P) for _ in range(6)] + [1, P - 1]
    w = lambda v: np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)], dtype=np.uint32)  # noqa: E731
    a = np.ascontiguousarray(np.stack([w(v * R % P) for v in vals]))  # Montgomery form
    out = np.zeros_like(a)
    lib.tbls_hostsim_coop_sqrt_cand(a.ctypes.data, out.ctypes.data, len(vals))
    for v, r in zip(vals, out):
        m = sum(int(r[i]) << (32 * i) for i in range(12)) * RINV % P
        assert m == pow(v, (P + 1) // 4, P)


def test_coop_reduce(lib):
    """creduce64: sums of up to 64 product outputs (64-bit digit sums, |v| up to
    2^395) -> T = 1 digits with |v| < 1.6 p, same residue; both signs at the
    2^395 limit and values next to (q + 1/2) p."""
    X = C.reduce_cases()
    x = np.ascontiguousarray(np.array(X, dtype=np.int64))
    out = np.zeros((len(X), 16), dtype=np.int32)
    lib.tbls_hostsim_coop_reduce(x.ctypes.data, out.ctypes.data, len(X))
    C.check_reduce(X, out)


def test_coop_inv_raw(lib):
    """inv_row_lane0 on raw limbs over its whole contract ([0, 2p) without the
    raw value p): z < 2p, z == A^-1 R^2; the form with the early exit returns
    the same limbs."""
    A = C.inv_cases()
    a = _word_rows(A)
    outs = []
    for u in (0, 1):
        out = np.zeros_like(a)
        lib.tbls_hostsim_coop_inv_raw(u, a.ctypes.data, out.ctypes.data, len(A))
        outs.append([_unwords(r) for r in out])
    C.check_inv(A, outs[0])
    assert outs[1] == outs[0]


# ---- point arithmetic (tb_cpoint.h) -----------------------------------------
def _mont(v):
    return v * R % P


def _cpoint(lib, group, op, k, A, B):
    """Jacobian (X, Y, Z) per record as plain residues."""
    n = len(A)
    if group == 1:
        inp = np.array([w for a, b in zip(A, B) for v in (a[0], a[1], b[0], b[1]) for w in _words(_mont(v))], dtype=np.uint32)
        out = np.zeros(36 * n, dtype=np.uint32)
        lib.tbls_hostsim_cpoint_g1(op, inp.ctypes.data, out.ctypes.data, n, k)
        return [tuple(_unwords(out[36 * i + 12 * j : 36 * i + 12 * j + 12]) * RINV % P for j in range(3)) for i in range(n)]
    inp = np.array([w for a, b in zip(A, B) for v in (a[0], a[1], b[0], b[1]) for c in v for w in _words(_mont(c))], dtype=np.uint32)
    out = np.zeros(72 * n, dtype=np.uint32)
    lib.tbls_hostsim_cpoint_g2(op, inp.ctypes.data, out.ctypes.data, n, k)
    res = []
    for i in range(n):
        c = [_unwords(out[72 * i + 12 * j : 72 * i + 12 * j + 12]) * RINV % P for j in range(6)]
        res.append(((c[0], c[1]), (c[2], c[3]), (c[4], c[5])))
    return res


@pytest.mark.parametrize("op", C.G1_OPS)
def test_cpoint_g1(lib, op):
    A, B, k = C.point_cases(1, op)
    C.check_points(1, op, A, B, k, _cpoint(lib, 1, op, k, A, B))


@pytest.mark.parametrize("op", C.G2_OPS)
def test_cpoint_g2(lib, op):
    A, B, k = C.point_cases(2, op)
    C.check_points(2, op, A, B, k, _cpoint(lib, 2, op, k, A, B))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("op", C.EXCEPTIONAL_OPS)
def test_cpoint_exceptional(lib, group, op):
    """P == +-Q, an infinite operand and doubling an infinite point give
    Z == 0 (mod p) without branches (tb_cpoint.h; tb_ccurve.h relies on it)."""
    A, B = C.exceptional_cases(group)
    C.check_exceptional(group, op, _cpoint(lib, group, op, 0, A, B))
