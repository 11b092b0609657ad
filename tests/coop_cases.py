"""Shared vectors and checks of the lane-cooperative row arithmetic
(teku_amd/csrc/tb_coop.h, tb_cinv.h, tb_cpoint.h).

tests/test_coop.py runs them on the host emulation of a 16-lane row and
tests/test_gpu_coop.py on the GPU (the DPP code), so both see identical inputs
and identical checks.  The generators are seeded and return plain Python
integers; the checkers take the inputs and whatever came back and compare with
Python-integer arithmetic only -- neither knows how a result was computed.
All checks are exact: no tolerances.
"""

import hashlib
import json
import os
import random

import numpy as np

from oracle import bls12_381 as O

P = O.P
R = 1 << 406  # tb_fp.h Montgomery radix
RINV = pow(R, -1, P)

GOLDEN_MUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coop_mul_digits.json")


# ---- digits -----------------------------------------------------------------
def val(d):
    """Value of a digit vector (radix 2^29, lanes 14 and 15 carry nothing)."""
    return sum(int(x) << (29 * j) for j, x in enumerate(d[:14]))


def balanced(v):
    """v as 13 balanced 29-bit digits ([-2^28, 2^28)) and the rest in digit 13."""
    d = []
    for _ in range(13):
        lo = ((v + (1 << 28)) & ((1 << 29) - 1)) - (1 << 28)
        d.append(lo)
        v = (v - lo) >> 29
    return d + [v, 0, 0]


def rnd_digits(rng, T, top=31, worst=False):
    """14 digits of class T (|d| <= T 2^28), lanes 14, 15 zero."""
    lim = T << 28
    if worst:
        d = [rng.choice((-lim, lim - 1)) for _ in range(13)]
    else:
        d = [rng.randint(-lim, lim - 1) for _ in range(13)]
    return d + [rng.randint(-top, top), 0, 0]


def digest(*digit_arrays):
    """SHA-256 of digit arrays as little-endian int32, in order."""
    h = hashlib.sha256()
    for a in digit_arrays:
        h.update(np.ascontiguousarray(np.array(a, dtype="<i4")).tobytes())
    return h.hexdigest()


def golden_mul():
    with open(GOLDEN_MUL) as f:
        return json.load(f)


# ---- product (cmul) ---------------------------------------------------------
MUL_CLASS_PAIRS = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (1, 2), (2, 2)]


def mul_class_cases(ta, tb):
    """300 random and 300 worst-case operand pairs of digit classes (ta, tb):
    T_a T_b <= 7 is the product's contract."""
    rng = random.Random(1000 * ta + tb)
    A, B = [], []
    for worst in (False, True):
        A += [rnd_digits(rng, ta, worst=worst) for _ in range(300)]
        B += [rnd_digits(rng, tb, worst=worst) for _ in range(300)]
    return A, B


def check_mul(A, B, out):
    """cmul's contract: T = 1 output digits, |v| < 1.01 p, v == a b / R (mod p)."""
    assert len(out) == len(A) == len(B)
    for a, b, r in zip(A, B, out):
        assert r[14] == 0 and r[15] == 0
        assert all(abs(int(x)) <= (1 << 28) + 8 for x in r[:13]), "output digit class"
        assert abs(int(r[13])) < 32, "output top digit"
        v = val(r)
        assert abs(v) < P + P // 100
        assert (v - val(a) * val(b) * RINV) % P == 0


def mul_chain(mul):
    """Outputs fed back as operands for 30 steps, then a sum of 7 outputs times
    an output; mul(A, B) -> digit rows.  Every step is checked; returns all
    the outputs, in order (for the digest)."""
    rng = random.Random(7)
    x = [rnd_digits(rng, 1) for _ in range(64)]
    y = [rnd_digits(rng, 1) for _ in range(64)]
    outs = []
    for _ in range(30):
        z = [list(map(int, r)) for r in mul(x, y)]
        check_mul(x, y, z)
        outs.append(z)
        x, y = y, z
    s = [[sum(int(r[j]) for r in (x[i], y[i], x[i], y[i], x[i], y[i], x[i])) for j in range(16)] for i in range(64)]
    z = [list(map(int, r)) for r in mul(s, y)]
    check_mul(s, y, z)
    outs.append(z)
    return outs


# ---- conversions ------------------------------------------------------------
def words_roundtrip_cases():
    """[0, 2p) 12-word operands, edges included (p, p + 1, 2p - 1)."""
    rng = random.Random(3)
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1] + [rng.randrange(2 * P) for _ in range(200)]
    return vals, list(reversed(vals))


def check_mul_words(A, B, out):
    """cfrom_words / cmul / cdigits_to_fp: fp_mul's residue, back in [0, 2p)."""
    assert len(out) == len(A)
    for x, y, v in zip(A, B, out):
        assert 0 <= v < 2 * P
        assert v % P == x * y * RINV % P


def to_fp_signed_cases():
    """Signed digit vectors of |value| < 64p."""
    rng = random.Random(4)
    D = []
    for _ in range(300):
        v = rng.choice([rng.randrange(-64 * P + 1, 64 * P), rng.randrange(-P, P), -64 * P + 1, 64 * P - 1])
        D.append(balanced(v))
    return D


def check_to_fp(D, out):
    assert len(out) == len(D)
    for dd, v in zip(D, out):
        assert 0 <= v < 2 * P and v % P == val(dd) % P


def zero_residue_cases():
    """Every multiple k p, |k| <= 64, as balanced digits: cdigits_to_fp must
    return exactly 0 (never p) -- the row inversion's callers rely on it."""
    return [balanced(k * P) for k in range(-64, 65)]


def check_zero_residues(D, out):
    assert len(out) == len(D) == 129
    for dd, v in zip(D, out):
        assert val(dd) % P == 0
        assert v == 0, "k p -> %d p" % (v // P) if v % P == 0 else "k p -> a non-zero residue"


# ---- creduce64 --------------------------------------------------------------
def _fat(rng, v, mag):
    """v as 64-bit digit sums: the 13 low digits random up to +-mag (what lazy
    sums of products look like), the top digit takes the rest."""
    d = [rng.randint(-mag, mag) for _ in range(13)]
    rest = v - sum(x << (29 * j) for j, x in enumerate(d))
    lo = balanced(rest)
    return [a + b for a, b in zip(d, lo[:13])] + [lo[13], 0, 0]


def reduce_cases():
    """64-bit digit sums within creduce64's contract (|digit sum| < 2^40,
    |v| < 2^395): sums of product outputs, both signs at the 2^395 limit, and
    values v ~ (q + 1/2) p for small and large q, where the rounded float
    estimate of v / p decides which way q goes."""
    rng = random.Random(11)
    X = []
    for _ in range(400):
        k = rng.choice([1, 2, 8, 36, 64, 4096])
        d = [sum(rng.randint(-(1 << 28), 1 << 28) for _ in range(min(k, 8))) * max(1, k // 8) for _ in range(13)]
        top = rng.randint(-(1 << 5), 1 << 5) * k
        X.append(d + [top, 0, 0])
    lim = 1 << 395
    for sign in (1, -1):
        for off in (1, 2, 1 << 29, 1 << 348, 1 << 377, P, rng.randrange(1 << 394), rng.randrange(1 << 394)):
            v = sign * (lim - off)
            X.append(balanced(v))
            X.append(_fat(rng, v, (1 << 39) - 1))
    qs = [0, 1, 2, 3, 7, 100, 1000, 4095, 4096, 8191, 12345, 16383, 20000, lim // P - 1]
    for q in qs:
        for sign in (1, -1):
            for delta in (0, 1, -1, P >> 40, -(P >> 40), P >> 24, -(P >> 24)):
                v = sign * ((2 * q + 1) * P // 2) + delta
                assert abs(v) < lim
                X.append(balanced(v))
                X.append(_fat(rng, v, (1 << 36)))
    for a in X:
        assert all(abs(x) < (1 << 40) for x in a) and abs(val(a)) < lim
    return X


def check_reduce(X, out):
    """creduce64's contract: T = 1 digits (|d| <= 2^28 + 2^12), lanes 14, 15
    zero, |v| < 1.6 p, same residue."""
    assert len(out) == len(X)
    for a, r in zip(X, out):
        assert r[14] == 0 and r[15] == 0
        assert all(abs(int(v)) <= (1 << 28) + (1 << 12) for v in r[:13])
        assert 10 * abs(val(r)) < 16 * P
        assert (val(r) - val(a)) % P == 0


# ---- row inversion (tb_cinv.h) ----------------------------------------------
def inv_edge_cases():
    """Raw inputs in [0, 2p) except p itself (outside inv_row_lane0's
    contract: its callers pass cdigits_to_fp's output, see zero_residue_cases)."""
    return [0, 1, 2, P - 1, P - 2, 1 << 380, P + 1, 2 * P - 1, 2 * P - 2, (1 << 381) + 12345, (1 << 381) + 1, 1 << 381]


def inv_cases():
    rng = random.Random(1234)
    A = [rng.randrange(P) for _ in range(100)] + [0, 1, 2, P - 1, P - 2, 1 << 380]
    A += [rng.randrange(1 << rng.randrange(1, 381)) for _ in range(30)]  # short values: long runs of zero bits
    A += inv_edge_cases()
    A += [rng.randrange(P, 2 * P) for _ in range(40)]
    A += [(1 << 381) + rng.randrange(1 << 20) for _ in range(4)]
    assert all(0 <= a < 2 * P and a != P for a in A)
    return A


def check_inv(A, out):
    """Raw limbs in, raw limbs out: z < 2p, z == A^-1 R^2 (mod p); 0 -> 0."""
    assert len(out) == len(A)
    for a, z in zip(A, out):
        assert 0 <= z < 2 * P
        if a % P == 0:
            assert a == 0 and z == 0
        else:
            assert z % P == pow(a, -1, P) * R * R % P, hex(a)


# ---- row point arithmetic (tb_cpoint.h) -------------------------------------
G1_OPS = [0, 1, 2, 3, 4, 5]
G2_OPS = [0, 1, 2, 3, 4]
EXCEPTIONAL_OPS = [8, 9, 10, 11, 12, 13, 14]  # tests/native/tb_cpoint_ops.h


def _field(group):
    return O.FP if group == 1 else O.FP2


def _points(group, rng, k):
    F, gen = (O.FP, O.G1_GEN) if group == 1 else (O.FP2, O.G2_GEN)
    return [O.jac_to_affine(F, O.jac_mul(F, O.jac_from_affine(F, gen), rng.randrange(1, O.R))) for _ in range(k)]


def point_cases(group, op):
    """(A, B, k): affine points P1, P2 per record and the launch's scalar."""
    if group == 1:
        rng = random.Random(100 + op)
        A, B = _points(1, rng, 6), _points(1, rng, 6)
        k = O.X_ABS if op == 5 else rng.getrandbits(64) | (1 << 63)
    else:
        rng = random.Random(200 + op)
        A, B = _points(2, rng, 3), _points(2, rng, 3)
        k = O.X_ABS if op == 3 else (rng.getrandbits(64) | (1 << 63) if op == 4 else 0)
    return A, B, k


def check_points(group, op, A, B, k, out):
    """out: Jacobian (X, Y, Z) per record, plain residues."""
    F = _field(group)
    assert len(out) == len(A)
    for i, (a, b, got) in enumerate(zip(A, B, out)):
        ja, jb = O.jac_from_affine(F, a), O.jac_from_affine(F, b)
        exp = {
            0: lambda: O.jac_double(F, ja),
            1: lambda: O.jac_add(F, O.jac_double(F, ja), jb),
            2: lambda: O.jac_add(F, O.jac_double(F, ja), O.jac_double(F, jb)),
            3: lambda: O.jac_mul(F, ja, k),
            4: lambda: O.jac_mul(F, O.jac_double(F, ja), k),
            5: lambda: O.jac_mul(F, ja, k * k),
        }[op]()
        assert O.jac_to_affine(F, got) == O.jac_to_affine(F, exp), (group, op, i)


def exceptional_cases(group):
    """(A, B): P2 = 2 P1, so dbl(P1) and P2 are one point in two forms."""
    rng = random.Random(300 + group)
    F = _field(group)
    A = _points(group, rng, 4)
    B = [O.jac_to_affine(F, O.jac_double(F, O.jac_from_affine(F, a))) for a in A]
    return A, B


def check_exceptional(group, op, out):
    """P == +-Q, an infinite operand, doubling an infinite point: Z == 0 (mod p)."""
    zero = 0 if group == 1 else (0, 0)
    assert len(out) == 4
    for i, got in enumerate(out):
        assert got[2] == zero, (group, op, i)
