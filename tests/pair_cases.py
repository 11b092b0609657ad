"""Shared inputs and plain references of the Miller stage: the line kernels,
the accumulators, the Fp12 products, the segment combine and the settle
kernels.

tests/test_gpu_pair_stage.py feeds these to the product kernels through the
test library's hook (tests/native/k_test_pair.hip) and compares raw outputs;
tests/test_pair_cases.py checks the references against oracle/bls12_381.py
without a GPU (the reference lines multiply out to O.miller_loop, the
segmented accumulator recombines to the unsegmented one, the comparators
reject what they must), so a wrong reference cannot pass for a wrong kernel.

Everything is oracle/bls12_381.py integer arithmetic, seeded, and compared by
exact equality of canonical integers: device Fp limbs (12 little-endian 32-bit
words, Montgomery R = 2^406, weakly reduced) are canonicalised mod p on
decoding.  Two comparisons are exact without being equalities, both by
construction of the kernels:
  * the device's lines are projective -- each is the oracle's affine line
    times a nonzero Fp2 factor (-2YZ at a doubling step) -- so a device line
    matches when it is nonzero and its three 2x2 cross-products with the
    reference vanish (line_matches);
  * Miller values built from such lines equal the oracle's up to a nonzero
    Fp2 factor, which the final exponentiation kills: dev * ref^-1 has a
    nonzero Fp2 coefficient c0.c0 and ten zero coordinates beside it
    (same_up_to_fp2).
"""

import random

import numpy as np

from oracle import bls12_381 as O

P = O.P
R_MONT = 1 << 406  # tb_fp.h
RINV = pow(R_MONT, -1, P)
STEPS = 68  # TB_LINE_STEPS: 63 doubling + 5 addition steps of |x|
LINE_G = 18  # 16-byte words per line (3 Fp2 = 72 32-bit limbs)
F12_BYTES = 576
UNWRITTEN = 0xEE


# ---- the steps of the loop, from the bits of |x| --------------------------------
def _step_kinds():
    kinds = []
    for bit in bin(O.X_ABS)[3:]:
        kinds.append("dbl")
        if bit == "1":
            kinds.append("add")
    return kinds


STEP_KINDS = _step_kinds()
DBL_STEPS = frozenset(s for s, k in enumerate(STEP_KINDS) if k == "dbl")
assert len(STEP_KINDS) == STEPS and len(DBL_STEPS) == 63


def seg_bounds(j, nseg):
    """Segment j of nseg: steps [lo, hi)."""
    return STEPS * j // nseg, STEPS * (j + 1) // nseg


def doublings_in(lo, hi):
    return sum(1 for s in range(lo, hi) if s in DBL_STEPS)


# ---- device encodings ---------------------------------------------------------------
def dec_fp(b48):
    return int.from_bytes(b48, "little") * RINV % P


def enc_fp(v):
    return (v % P * R_MONT % P).to_bytes(48, "little")


def enc_fp2(a):
    return enc_fp(a[0]) + enc_fp(a[1])


def enc_g1(pt):
    return enc_fp(pt[0]) + enc_fp(pt[1])


def dec_g1(b96):
    return (dec_fp(b96[:48]), dec_fp(b96[48:96]))


def enc_g2(pt):
    return enc_fp2(pt[0]) + enc_fp2(pt[1])


def dec_g2(b192):
    v = [dec_fp(b192[48 * k : 48 * k + 48]) for k in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def f12_flat(f):
    return [c for f6 in f for x in f6 for c in x]


def f12_unflat(v):
    x = [(v[2 * k], v[2 * k + 1]) for k in range(6)]
    return ((x[0], x[1], x[2]), (x[3], x[4], x[5]))


def enc_f12(f):
    return b"".join(enc_fp(c) for c in f12_flat(f))


def dec_f12(b576):
    return f12_unflat([dec_fp(b576[48 * k : 48 * k + 48]) for k in range(12)])


def dec_f12s(raw, count):
    """`count` consecutive Fp12 values; None where all 576 bytes are unwritten."""
    out = []
    for k in range(count):
        b = raw[F12_BYTES * k : F12_BYTES * (k + 1)]
        out.append(None if b == bytes([UNWRITTEN]) * F12_BYTES else dec_f12(b))
    return out


def enc_line_table(lines_of_pair):
    """lines_of_pair[i][s] = (a, b, c) in Fp2 -> the structure-of-arrays table of
    tb_lines.h line_store: word (s * 18 + g) * n + i holds 16-byte group g of
    line s of pair i (a.c0, a.c1, b.c0, b.c1, c.c0, c.c1; 48 bytes each).  A
    pair given as None keeps 0xEE in all its slots."""
    n = len(lines_of_pair)
    t = np.full((STEPS, LINE_G, n, 16), UNWRITTEN, dtype=np.uint8)
    for i, lines in enumerate(lines_of_pair):
        if lines is None:
            continue
        for s, (a, b, c) in enumerate(lines):
            raw = enc_fp2(a) + enc_fp2(b) + enc_fp2(c)
            t[s, :, i, :] = np.frombuffer(raw, dtype=np.uint8).reshape(LINE_G, 16)
    return t.tobytes()


def dec_line_table(raw, n):
    """The inverse: [pair][step] -> (a, b, c), or None for a slot that is still
    0xEE in all its 288 bytes."""
    t = np.frombuffer(raw, dtype=np.uint8)[: STEPS * LINE_G * n * 16].reshape(STEPS, LINE_G, n, 16)
    out = []
    for i in range(n):
        col = t[:, :, i, :].reshape(STEPS, 288)
        lines = []
        for s in range(STEPS):
            b = col[s].tobytes()
            if b == bytes([UNWRITTEN]) * 288:
                lines.append(None)
                continue
            v = [dec_fp(b[48 * k : 48 * k + 48]) for k in range(6)]
            lines.append(((v[0], v[1]), (v[2], v[3]), (v[4], v[5])))
        out.append(lines)
    return out


# ---- reference lines -------------------------------------------------------------------
def ref_lines(p_aff, q_aff):
    """The 68 affine lines (A, B, C) of O.miller_loop(p_aff, q_aff), step by
    step as it computes them: A = lambda x_T - y_T, B = -lambda x_P, C = y_P."""
    xp, yp = p_aff
    xq, yq = q_aff
    tx, ty = xq, yq
    C = (yp % P, 0)
    out = []
    for kind in STEP_KINDS:
        if kind == "dbl":
            lam = O.f2_mul(O.f2_mul_fp(O.f2_sqr(tx), 3), O.f2_inv(O.f2_add(ty, ty)))
            nx = O.f2_sub(O.f2_sqr(lam), O.f2_add(tx, tx))
        else:
            lam = O.f2_mul(O.f2_sub(yq, ty), O.f2_inv(O.f2_sub(xq, tx)))
            nx = O.f2_sub(O.f2_sub(O.f2_sqr(lam), tx), xq)
        out.append((O.f2_sub(O.f2_mul(lam, tx), ty), O.f2_neg(O.f2_mul_fp(lam, xp)), C))
        ty = O.f2_sub(O.f2_mul(lam, O.f2_sub(tx, nx)), ty)
        tx = nx
    return out


def line_matches(dev, ref):
    """dev = k ref for a nonzero k in Fp2: dev is nonzero and the three 2x2
    cross-products vanish (ref is never zero: its C is y_P)."""
    if dev is None or all(O.f2_is_zero(x) for x in dev):
        return False
    for i, j in ((0, 1), (0, 2), (1, 2)):
        if not O.f2_is_zero(O.f2_sub(O.f2_mul(dev[i], ref[j]), O.f2_mul(dev[j], ref[i]))):
            return False
    return True


def line_mismatch(dev_lines, ref):
    """The first (step, coefficient pair) at which a pair's device lines do not
    match the reference projectively, or None."""
    for s in range(STEPS):
        d = dev_lines[s]
        if d is None:
            return (s, "unwritten")
        if all(O.f2_is_zero(x) for x in d):
            return (s, "zero line")
        for i, j in ((0, 1), (0, 2), (1, 2)):
            if not O.f2_is_zero(O.f2_sub(O.f2_mul(d[i], ref[s][j]), O.f2_mul(d[j], ref[s][i]))):
                return (s, "abc"[i] + "abc"[j])
    return None


# ---- reference accumulator ------------------------------------------------------------
def line_f12(line):
    """(a, b, c) as the sparse Fp12 element (a + b v) + (c v) w."""
    a, b, c = line
    return ((a, b, O.F2_ZERO), (O.F2_ZERO, c, O.F2_ZERO))


def ref_segment(columns, lo, hi):
    """Steps [lo, hi) over the line columns of a group's valid pairs, from
    f = 1: f <- f^2 at a doubling step, then f <- f * line for every column;
    i.e. prod_s (prod_k line_{k,s})^(2^(doubling steps after s in the segment)).
    Not conjugated."""
    f = O.F12_ONE
    for s in range(lo, hi):
        if s in DBL_STEPS:
            f = O.f12_sqr(f)
        for col in columns:
            f = O.f12_mul(f, line_f12(col[s]))
    return f


def ref_acc(lines_of_pair, valid, groups, nseg):
    """out[j][g] = conj(segment j of group g) as the kernels store it.
    groups[g]: the pairs group g owns; valid[i]: pair i is not killed."""
    out = []
    for j in range(nseg):
        lo, hi = seg_bounds(j, nseg)
        out.append([O.f12_conj(ref_segment([lines_of_pair[i] for i in own if valid[i]], lo, hi)) for own in groups])
    return out


def groups_contiguous(n, per):
    """k_miller_acc1/2: thread t owns pairs per t .. per t + per - 1."""
    return [list(range(per * t, min(n, per * t + per))) for t in range((n + per - 1) // per)]


def groups_strided(n, per):
    """k_miller_accs_lds: group g owns g, g + G, g + 2G, ... with G = ceil(n / per)."""
    G = (n + per - 1) // per
    return [[g + k * G for k in range(per) if g + k * G < n] for g in range(G)]


def ref_combine(vals):
    """The Horner combine over segment values (stored form): R = v_0, then
    R = R^(2^d_j) v_j with d_j the doubling steps of segment j.  Equals
    prod_j v_j^(2^D_j), D_j the doubling steps after segment j."""
    nseg = len(vals)
    r = vals[0]
    for j in range(1, nseg):
        for _ in range(doublings_in(*seg_bounds(j, nseg))):
            r = O.f12_sqr(r)
        r = O.f12_mul(r, vals[j])
    return r


def ref_unsegmented(vals):
    """prod_j v_j^(2^D_j) from the definition (the combine's cross-check)."""
    nseg = len(vals)
    r = O.F12_ONE
    for j, v in enumerate(vals):
        r = O.f12_mul(r, O.f12_pow(v, 1 << doublings_in(seg_bounds(j, nseg)[1], STEPS)))
    return r


def ref_product(vals):
    r = vals[0]
    for v in vals[1:]:
        r = O.f12_mul(r, v)
    return r


def fp2_defect(dev, ref):
    """None when dev = k ref for a nonzero k in Fp2 -- the exact condition under
    which the two pair alike: dev * ref^-1 has c0.c0 != 0 and its ten other Fp
    coordinates zero -- else the index of the first offending coordinate."""
    flat = f12_flat(O.f12_mul(dev, O.f12_inv(ref)))
    return ratio_defect(flat)


def ratio_defect(flat):
    if flat[0] == 0 and flat[1] == 0:
        return 0
    for k in range(2, 12):
        if flat[k] != 0:
            return k
    return None


def same_up_to_fp2(dev, ref):
    return fp2_defect(dev, ref) is None


# ---- pairs and sets -----------------------------------------------------------------------
def g1_mul(k):
    return O.jac_to_affine(O.FP, O.jac_mul(O.FP, O.jac_from_affine(O.FP, O.G1_GEN), k % O.R))


def g2_mul(k):
    return O.jac_to_affine(O.FP2, O.jac_mul(O.FP2, O.jac_from_affine(O.FP2, O.G2_GEN), k % O.R))


def g1_neg(pt):
    return (pt[0], (-pt[1]) % P)


HASH_MSGS = (b"pair-cases: first hashed point", b"pair-cases: second hashed point")


def real_pairs(n, seed=41):
    """n pairs (P, Q, e): P = [a] g1 and Q = [b] g2 with small a, b, e = a b (the
    pair's pairing is e(g1, g2)^e); the last four are (g1, H_0), (-g1, H_0),
    (g1, H_1), (-g1, H_1) on hashed points, e = None."""
    rng = random.Random(seed)
    out = []
    for _ in range(n - 4):
        a, b = rng.randrange(1, 200), rng.randrange(1, 200)
        out.append((g1_mul(a), g2_mul(b), a * b))
    for m in HASH_MSGS:
        h = O.hash_to_g2(m)
        out.append((O.G1_GEN, h, None))
        out.append((O.NEG_G1, h, None))
    return out


def settle_sets(n, forged, seed=43):
    """n sets as 2n pairs in the settle layout: pair g is ([r sk] g1, [b] g2)
    -- the set's (r apk, H(m)) -- and pair n + g is (-[r] g1, [sk b] g2) -- its
    (-r g1, sig); a forged set signs with sk + 1.  Returns (P list, Q list)."""
    rng = random.Random(seed)
    Ps, Qs = [None] * (2 * n), [None] * (2 * n)
    for g in range(n):
        sk, b, r = rng.randrange(2, 1 << 20), rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 20)
        Ps[g], Qs[g] = g1_mul(r * sk), g2_mul(b)
        Ps[n + g], Qs[n + g] = g1_neg(g1_mul(r)), g2_mul((sk + 1 if g in forged else sk) * b)
    return Ps, Qs


# ---- synthetic tables and flags --------------------------------------------------------------
EDGE_FP = (0, 1, P - 1)


def random_fp(rng):
    return rng.choice(EDGE_FP) if rng.random() < 0.08 else rng.randrange(P)


def random_fp2(rng):
    return (random_fp(rng), random_fp(rng))


def random_lines(n, seed):
    """n columns of 68 lines of seeded random Fp coefficients, some of them 0, 1
    and p - 1."""
    rng = random.Random(seed)
    return [[(random_fp2(rng), random_fp2(rng), random_fp2(rng)) for _ in range(STEPS)] for _ in range(n)]


def random_f12(rng):
    return f12_unflat([random_fp(rng) for _ in range(12)])


def random_f12_values(count, seed):
    """Random Fp12 values (about one coordinate in twelve is 0, 1 or p - 1) with
    the identity and values of twelve coordinates p - 1 among them."""
    rng = random.Random(seed)
    out = [random_f12(rng) for _ in range(count)]
    if count > 8:
        out[1] = O.F12_ONE
        out[3] = out[count - 2] = f12_unflat([P - 1] * 12)
    return out


def kill_flags(n, groups, seed):
    """(skip, code_a, code_b) byte lists for n pairs.  Groups 0 .. 4 (as far as
    they exist) get 0, 1, 2, 3 and all of their pairs valid, the valid ones
    drawn at random so the mask has holes; elsewhere about a quarter of the
    pairs are killed, split across the three arrays."""
    rng = random.Random(seed)
    flags = [[0] * n for _ in range(3)]
    special = set()
    for g, want in zip(range(min(5, len(groups))), (0, 1, 2, 3, None)):
        own = groups[g]
        special.update(own)
        keep = set(own) if want is None else set(rng.sample(own, min(want, len(own))))
        for i in own:
            if i not in keep:
                flags[rng.randrange(3)][i] = rng.choice((1, 2, 0xFF))
    for i in range(n):
        if i not in special and rng.random() < 0.25:
            flags[rng.randrange(3)][i] = rng.choice((1, 2, 0xFF))
    return tuple(flags)


def valid_of(flags):
    skip, ca, cb = flags
    return [s == 0 and a == 0 and b == 0 for s, a, b in zip(skip, ca, cb)]
