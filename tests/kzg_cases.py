"""Shared cases and checks of the KZG device code's scalar side (teku_amd/csrc/
tb_fr.h, tb_glv.h) and of its point and term kernels (k_kzg.hip).

tests/test_kzg_ops.py runs the primitive ops on the host build and
tests/test_gpu_kzg_ops.py on the GPU, with identical inputs and identical
checks; tests/test_gpu_kzg_kernels.py uses the point and term cases.  The
generators are seeded; every expected value is Python-integer arithmetic or the
Python oracle (oracle/bls12_381.py).  All checks are exact: no tolerances.
"""

import functools
import os
import random
import re

from oracle import bls12_381 as O

R = O.R
MU = O.X_ABS**2  # the GLV eigenvalue: r = mu^2 - mu + 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def consts():
    """FR_MOD, FR_R2, FR_OMEGA (plain), GLV_MU, GLV_M as the kernels have them
    (little-endian 32-bit limbs of teku_amd/csrc/tb_consts.h)."""
    src = open(os.path.join(ROOT, "teku_amd", "csrc", "tb_consts.h")).read()

    def val(name):
        m = re.search(r"TB_CONST uint32_t " + name + r"\[\d+\] = \{([^}]*)\}", src)
        return sum(int(x.strip().rstrip("u"), 16) << (32 * i) for i, x in enumerate(m.group(1).split(",")))

    rinv = pow(1 << 256, -1, R)
    return {"FR_MOD": val("FR_MOD"), "FR_R2": val("FR_R2"), "FR_OMEGA": val("FR_OMEGA_M") * rinv % R, "GLV_MU": val("GLV_MU"),
            "GLV_M": val("GLV_M")}


def be32(v):
    return int(v).to_bytes(32, "big")


def i32(b):
    return int.from_bytes(b[:32], "big")


def fr_out(o):
    """An Fr result record: the value, after asserting the op's own limbs were
    fully reduced (byte 32; the conversion to bytes would hide a result >= r)."""
    assert o[32] == 1, "result limbs not below r"
    return i32(o)


# ---- Fr ---------------------------------------------------------------------
FR_EDGE = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, ((1 << 255) - 1) % R, (1 << 32) - 1, 1 << 224]


def fr_pairs():
    rng = random.Random(4844)
    return [(a, b) for a in FR_EDGE for b in FR_EDGE] + [(rng.randrange(R), rng.randrange(R)) for _ in range(64)]


def check_fr_arith(run):
    """FR_ADD / SUB / MUL / SQR / NEG: the result, its limbs fully reduced."""
    pairs = fr_pairs()
    recs = [be32(a) + be32(b) for a, b in pairs]
    for op, f in [("FR_ADD", lambda a, b: (a + b) % R), ("FR_SUB", lambda a, b: (a - b) % R), ("FR_MUL", lambda a, b: a * b % R),
                  ("FR_SQR", lambda a, b: a * a % R), ("FR_NEG", lambda a, b: -a % R)]:
        out = run(op, recs)
        loose = [(hex(a), hex(b)) for (a, b), o in zip(pairs, out) if o[32] != 1]
        assert not loose, (op, "limbs not below r", loose[:4])
        got = [i32(o) for o in out]
        want = [f(a, b) for a, b in pairs]
        bad = [(hex(a), hex(b)) for (a, b), g, w in zip(pairs, got, want) if g != w]
        assert not bad, (op, bad[:4])


def fr_mul_raw_cases():
    rng = random.Random(4845)
    top = 1 << 256
    A = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, top - R, top - 1]
    B = [0, 1, R - 1, consts()["FR_R2"], rng.randrange(R)]
    return [(a, b) for a in A for b in B]


def check_fr_mul_raw(run):
    """fr_from_digest's contract: one operand anywhere below 2^256, the other
    below r -- the CIOS product comes out as a b 2^-256 mod r, fully reduced."""
    cases = fr_mul_raw_cases()
    rinv = pow(1 << 256, -1, R)
    out = run("FR_MUL_RAW", [be32(a) + be32(b) for a, b in cases])
    for (a, b), o in zip(cases, out):
        raw = i32(o)
        assert raw < R, (hex(a), hex(b), hex(raw))
        assert raw == a * b * rinv % R, (hex(a), hex(b))


def check_fr_inv(run):
    rng = random.Random(4846)
    A = [0, 1, 2, R - 1, R - 2] + [1 << k for k in (31, 32, 33, 254)] + [rng.randrange(R) for _ in range(16)]
    got = [fr_out(o) for o in run("FR_INV", [be32(a) for a in A])]
    assert got == [pow(a, -1, R) if a else 0 for a in A]


def check_fr_pow_u32(run):
    rng = random.Random(4847)
    E = [0, 1, 2, 4095, 4096, 1 << 31, (1 << 32) - 1]
    A = [0, 1, consts()["FR_OMEGA"], rng.randrange(R)]
    assert pow(A[2], 4096, R) == 1 and pow(A[2], 2048, R) != 1  # the parsed constant is the 4096th root
    cases = [(a, e) for a in A for e in E]
    got = [fr_out(o) for o in run("FR_POW_U32", [be32(a) + e.to_bytes(4, "little") for a, e in cases])]
    assert got == [pow(a, e, R) for a, e in cases]


def check_fr_from_bytes(run):
    """spec bytes_to_bls_field: canonical or rejected; accepted values round-trip."""
    V = [R - 1, R, R + 1, (1 << 256) - 1, 1 << 255, 0]
    out = run("FR_FROM_BYTES", [be32(v) for v in V])
    for v, o in zip(V, out):
        flag = int.from_bytes(o[:4], "little")
        assert flag == (1 if v < R else 0), hex(v)
        if v < R:
            assert i32(o[4:36]) == v, hex(v)


def check_fr_from_digest(run):
    rng = random.Random(4848)
    V = [0, R - 1, R, R + 1, 2 * R, 2 * R + 1, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(16)]
    got = [fr_out(o) for o in run("FR_FROM_DIGEST", [be32(v) for v in V])]
    assert got == [v % R for v in V]


# ---- GLV --------------------------------------------------------------------
def glv_cases():
    """The scalars of the GLV_SPLIT check.  The last line adds eight multiples
    of mu with chosen cofactors to the seeded ones, so that more than 40 cases
    need the correction."""
    rng = random.Random(4849)
    ks = [0, 1, MU - 1, MU, MU + 1, 2 * MU - 1, 2 * MU, R - 1, R - 2]
    for _ in range(32):
        j = rng.randrange(MU)
        ks += [j * MU, j * MU + 1, j * MU + 2, j * MU + 3, j * MU - 1]
    ks += [rng.randrange(R) for _ in range(64)]
    ks += [(1 << k) - 1 for k in range(1, 255)]
    ks += [j * MU for j in (3, 1 << 32, (1 << 64) - 1, 1 << 64, 1 << 96, 1 << 127, MU - 2, MU // 2)]
    assert all(0 <= k < R for k in ks)
    return ks


def glv_corrections(k):
    """How many times glv_split must subtract mu after its quotient estimate."""
    c = consts()
    return k // c["GLV_MU"] - ((k * c["GLV_M"]) >> 384)


def check_glv_split(run):
    c = consts()
    assert c["GLV_MU"] == MU and c["GLV_M"] == (1 << 384) // MU and c["FR_MOD"] == R and R == MU * MU - MU + 1
    ks = glv_cases()
    classes = [glv_corrections(k) for k in ks]
    assert classes.count(0) >= 40 and classes.count(1) >= 40, (classes.count(0), classes.count(1))
    assert set(classes) <= {0, 1}, sorted(set(classes))  # never 2: the estimate's error is below k / 2^384 < 1
    assert all(glv_corrections(k) == 1 for k in (MU, R - 1)) and glv_corrections(MU - 1) == 0
    out = run("GLV_SPLIT", [be32(k) for k in ks])
    for k, o in zip(ks, out):
        a, b = int.from_bytes(o[:16], "big"), int.from_bytes(o[16:32], "big")
        assert a + b * MU == k, hex(k)
        assert a < MU and b < (1 << 128), hex(k)


@functools.lru_cache(maxsize=None)
def mul_scalars():
    """The scalar list of G1_MUL_FR (also the z_i of the term kernels and the
    chosen scalars of the constructed relation in tests/test_gpu_kzg.py)."""
    rng = random.Random(4850)
    ks = [0, 1, 2, 3, MU - 1, MU, MU + 1, 2 * MU, R - 1, R - 2, 1 << 127, (1 << 128) - 1, 1 << 128]
    ks += [rng.randrange(MU) * MU for _ in range(8)]
    ks += [rng.randrange(R) for _ in range(16)]
    return tuple(ks)


def g1_mul(a, k):
    """[k]a affine (None: infinity) by the oracle's double-and-add."""
    return O.jac_to_affine(O.FP, O.jac_mul(O.FP, O.jac_from_affine(O.FP, a), k))


@functools.lru_cache(maxsize=None)
def mul_points():
    rng = random.Random(4851)
    return (O.G1_GEN, O.NEG_G1, g1_mul(O.G1_GEN, rng.randrange(1, R)), g1_mul(O.G1_GEN, rng.randrange(1, R)))


def enc_aff(a):
    return a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def dec_aff(b):
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


def check_g1_mul_fr(run):
    cases = [(P, k) for P in mul_points() for k in mul_scalars()]
    out = run("G1_MUL_FR", [enc_aff(P) + be32(k) for P, k in cases])
    for (P, k), o in zip(cases, out):
        want = g1_mul(P, k)
        fin = int.from_bytes(o[:4], "little")
        assert fin == (0 if want is None else 1), hex(k)
        if want is not None:
            assert dec_aff(o[4:100]) == want, hex(k)


CHECKS = [check_fr_arith, check_fr_mul_raw, check_fr_inv, check_fr_pow_u32, check_fr_from_bytes, check_fr_from_digest, check_glv_split,
          check_g1_mul_fr]


# ---- k_kzg_terms / k_kzg_terms_coop -------------------------------------------
@functools.lru_cache(maxsize=None)
def term_points():
    """Finite G1 points for commitments and proofs (the generator among them)."""
    rng = random.Random(4852)
    return (O.G1_GEN, O.NEG_G1) + tuple(g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(6))


def _ys_with_sum(rng, n, rr, target, fixed=None):
    """y with sum_i rr^i y_i == target: the others seeded (or `fixed`), y_0 solved."""
    ys = list(fixed) if fixed else [0] + [rng.randrange(1, R) for _ in range(n - 1)]
    ys[0] = (target - sum(pow(rr, i, R) * ys[i] for i in range(1, n))) % R
    return ys


def term_cases():
    """(n, commitments, proofs, inf flags (2n), z, y, r) per case.  z runs over
    mul_scalars() (so the GLV correction, scalar 0 and r - 1 reach both forms);
    r over {1, r - 1, mu, random}; sum r^i y_i over {r - 1, mu, random} and,
    in the first n = 3 case, 0 from non-zero terms; the infinity flags over
    none / a commitment / a proof / both."""
    rng = random.Random(4853)
    pts = term_points()
    ks = list(mul_scalars())
    cases = []
    for n in (1, 3):
        zs = ks + ks[: -len(ks) % n]
        for c in range(len(zs) // n):
            z = zs[n * c : n * c + n]
            r = [1, R - 1, MU, rng.randrange(R)][c % 4]
            rr = r if n > 1 else 1  # n == 1: r is ignored
            target = [R - 1, MU, rng.randrange(R)][c % 3]
            y = _ys_with_sum(rng, n, rr, target)
            com = [pts[(c + 2 * i) % len(pts)] for i in range(n)]
            prf = [pts[(c + 2 * i + 1) % len(pts)] for i in range(n)]
            inf = [0] * (2 * n)
            kind = (c // 4) % 4  # none, a commitment, a proof, both
            if kind in (1, 3):
                inf[c % n] = 1
            if kind in (2, 3):
                inf[n + (c + 1) % n] = 1
            cases.append((n, com, prf, inf, z, y, r))
    # sum r^i y_i = 0 with non-zero terms
    cases.append((3, list(pts[2:5]), list(pts[5:8]), [0] * 6, [ks[5], ks[8], ks[0]], [1, R - 1, 0], 1))
    return cases


def term_input(case):
    """The stage-1 input of tests/native/k_test_kzg.hip."""
    n, com, prf, inf, z, y, r = case
    return b"".join(enc_aff(a) for a in com + prf) + bytes(inf) + b"".join(be32(v) for v in z + y + [r])


def term_expected(case):
    """T[k] affine (None: infinity), k in [0, 3n], from the kernel's documented
    term list: [r^k] proof_k, [r^i] C_i, [r^i z_i] proof_i, [sum r^i y_i](-G1)."""
    n, com, prf, inf, z, y, r = case
    rr = r if n > 1 else 1
    rp = [pow(rr, i, R) for i in range(n)]
    T = [None if inf[n + i] else g1_mul(prf[i], rp[i]) for i in range(n)]
    T += [None if inf[i] else g1_mul(com[i], rp[i]) for i in range(n)]
    T += [None if inf[n + i] else g1_mul(prf[i], rp[i] * z[i] % R) for i in range(n)]
    T.append(g1_mul(O.NEG_G1, sum(rp[i] * y[i] for i in range(n)) % R))
    return T


def dec_term(rec):
    return dec_aff(rec[4:100]) if rec[0] else None


# ---- k_kzg_points / k_kzg_points_coop ----------------------------------------
@functools.lru_cache(maxsize=None)
def bad_points():
    """name -> 48 bytes the point kernels must reject (well-formed inputs)."""
    from tests.test_gpu_kcoop import bad_keys  # seeded; pure oracle arithmetic

    p_hdr = lambda v: bytes([0x80 | (v >> 376)]) + (v & ((1 << 376) - 1)).to_bytes(47, "big")  # noqa: E731
    x = 1
    while O.fp_sqrt((x * x * x + O.B_G1) % O.P) is not None:
        x += 1
    good = O.g1_compress(O.G1_GEN)
    out = {
        "infinity with the sign bit": bytes([0xE0]) + bytes(47),
        "infinity with a low byte": bytes([0xC0]) + bytes(46) + b"\x01",
        "compression bit clear": bytes([good[0] & 0x7F]) + good[1:],
        "x = p": p_hdr(O.P),
        "x = p + 1": p_hdr(O.P + 1),
        "x off the curve": bytes([0x80]) + x.to_bytes(48, "big")[1:],
        "x = 0": bytes([0x80]) + bytes(47),
        "x = 0, sign bit": bytes([0xA0]) + bytes(47),
    }
    out.update(bad_keys())  # a random on-curve point outside G1 and points of order 3, 11, 33
    return out


@functools.lru_cache(maxsize=None)
def good_points():
    """Valid encodings: finite points with either sign bit, and infinity."""
    rng = random.Random(4855)
    pts = [g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(5)]
    enc = [O.g1_compress(a) for a in pts] + [O.g1_compress((a[0], -a[1] % O.P)) for a in pts]
    assert {e[0] & 0x20 for e in enc} == {0, 0x20}
    return tuple(enc) + (O.INFINITY_G1,)


@functools.lru_cache(maxsize=None)
def point_expected(b):
    """(code, inf, affine-or-None) of k_kzg_points for 48 bytes: the oracle's
    decode code, then the subgroup check for a finite decoded point."""
    code, a = O.g1_decompress(b)
    if code == O.SUCCESS and a is not None and not O.g1_in_group(O.jac_from_affine(O.FP, a)):
        code = O.POINT_NOT_IN_GROUP
    return code, 1 if (code == O.SUCCESS and a is None) else 0, a if code == O.SUCCESS else None


POINT_COUNTS = (1, 2, 3, 4, 5, 9)  # the last 4-row workgroup has 1, 2 or 3 active rows


def point_batches():
    """(name, [48-byte encodings]) per launch: every count all valid, and every
    bad input once in each row position 0..3 (and in the last, partly filled
    workgroup) with valid points in the other rows."""
    good = good_points()
    out = []
    for m in POINT_COUNTS:
        out.append((f"m={m} valid", [good[(m + i) % len(good)] for i in range(m)]))
    for j, (name, b) in enumerate(bad_points().items()):
        for m in POINT_COUNTS:
            for pos in sorted(set(range(min(m, 4))) | {m - 1}):
                batch = [good[(j + m + i) % len(good)] for i in range(m)]
                batch[pos] = b
                out.append((f"m={m} {name} at {pos}", batch))
    return out


# ---- the host-side plans and entry points (tools/kzg_record.py) ---------------
FORM_SEEDS = (700, 701, 702, 703, 704)  # the batch's blobs (tests/kzg_util.py sample_blob)
FORM_OTHER_SEED = 705  # the blob whose proof stands in at n == 1
FORM_COUNTS = (1, 2, 3, 5)


def form_cases(blobs, cs, ps, other_proof):
    """(name, kind, blobs, commitments, proofs) per case from the five seeded
    blobs with their commitments and proofs.  kind: "valid", "false", or the
    BADARGS message verify_dev's loops give (the lowest offending index)."""
    bad_pt = bad_points()["order 11"]
    out = []
    for n in FORM_COUNTS:
        b, c, p = list(blobs[:n]), list(cs[:n]), list(ps[:n])
        out.append((f"n={n} valid", "valid", b, c, p))
        swapped = [other_proof] if n == 1 else [p[1], p[0]] + p[2:]
        out.append((f"n={n} wrong proofs", "false", b, c, swapped))
        out.append((f"n={n} order-11 commitment", f"Invalid commitment at index {n - 1}.", b, c[:-1] + [bad_pt], p))
        noncanon = b[-1][: 32 * 77] + be32(R) + b[-1][32 * 78 :]
        out.append((f"n={n} non-canonical element", f"Invalid blob at index {n - 1}: non-canonical field element.", b[:-1] + [noncanon], c, p))
    b, c, p = list(blobs[:3]), list(cs[:3]), list(ps[:3])
    out.append(("n=3 two bad proofs", "Invalid proof at index 1.", b, c, [p[0], bad_pt, bad_pt]))
    return out
