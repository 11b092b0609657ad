"""Shared inputs and plain reference of the key stage, the signature stage and
the hash kernel's randomizer branch of a randomized batch.

tests/test_gpu_stages.py feeds these to the product kernels through the test
library's hook (tests/native/k_test_stages.hip) and compares raw outputs;
tests/test_stage_cases.py checks the reference against itself without a GPU
(secret-key identities, sum_j [2^j] V_j = sum_i [r_i] sig_i), so a wrong
reference cannot pass for a wrong kernel.

The reference is oracle/bls12_381.py integer arithmetic: decode every point,
add, multiply.  The C oracle only makes inputs (keys and signatures from
secret keys).  Every secret key is kept beside its point, which is what the
CPU test's identities use.  Everything is seeded; every comparison is exact
equality of canonical integers.  Randomizers lie in [1, 2^64) -- never 0.
"""

import functools
import random
from collections import namedtuple

from oracle import bls12_381 as O
from oracle import c_oracle as C
from oracle.keys import interop_sk

P = O.P
RINV = pow(1 << 406, -1, P)  # Montgomery R = 2^406 (tb_fp.h)
M64 = (1 << 64) - 1
MSG = b"stage-cases: every signature here signs this one message"


# ---- decoding device values ---------------------------------------------------
def dec_fp(b48):
    """12 little-endian 32-bit limbs, Montgomery -> canonical integer."""
    return int.from_bytes(b48, "little") * RINV % P


def dec_g1(b96):
    """g1a -> (x, y); the kernels' 'no point' is (0, 0)."""
    return (dec_fp(b96[:48]), dec_fp(b96[48:96]))


def dec_g2(b192):
    """g2a (x.c0, x.c1, y.c0, y.c1) -> ((x0, x1), (y0, y1))."""
    v = [dec_fp(b192[48 * k : 48 * k + 48]) for k in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def dec_g2j(b288):
    """g2j (Jacobian X, Y, Z) -> affine or None."""
    v = [dec_fp(b288[48 * k : 48 * k + 48]) for k in range(6)]
    return O.jac_to_affine(O.FP2, ((v[0], v[1]), (v[2], v[3]), (v[4], v[5])))


ZERO_G1 = (0, 0)
ZERO_G2 = ((0, 0), (0, 0))


# ---- randomizers --------------------------------------------------------------
HOSTSIM_RANDS = [1, 2, 3, 4, 5, 7, 1 << 63, M64, 0x8000000000000001, 0x5555555555555555, 0xC000000000000003, 0x100000000]  # tests/test_hostsim.py
BYTE_RANDS = [d << (8 * w) for w in range(8) for d in (1, 255)]  # one non-zero byte: one comb / bucket entry
# the top 2-bit window digit 1 (an even top bit), 2 and 3 (an odd one), at the top and near the bottom
TOP_WINDOW_RANDS = [0x4000000000000001, 0x8000000000000001, 0xC000000000000001, 0x11, 0x21, 0x31]
OTHER_RANDS = [0xFF, 0x100, 0x101, 0x00FF00FF00FF00FF, 0xFF00FF00FF00FF00, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x0100000000000001]


def edge_rands():
    out = []
    for r in HOSTSIM_RANDS + BYTE_RANDS + OTHER_RANDS + TOP_WINDOW_RANDS:
        if r not in out:
            out.append(r)
    return out


def seeded_rands(seed, k):
    rng = random.Random(seed)
    return [rng.getrandbits(64) or 1 for _ in range(k)]


# ---- points from secret keys ---------------------------------------------------
_pk_cache, _sig_cache = {}, {}


def pk_of(sk):
    sk %= O.R
    if sk not in _pk_cache:
        _pk_cache[sk] = C.sk_to_pk(sk)
    return _pk_cache[sk]


def sig_of(sk):
    """[sk] H(MSG), compressed; sig_of(R - sk) is its negation."""
    sk %= O.R
    if sk not in _sig_cache:
        _sig_cache[sk] = C.sign(sk, MSG)
    return _sig_cache[sk]


def g1_of_bytes(b48):
    code, a = O.g1_decompress(b48)
    assert code == O.SUCCESS and a is not None
    return a


def g2_of_bytes(b96):
    code, a = O.g2_decompress(b96)
    assert code == O.SUCCESS and a is not None
    return a


def off_curve_key():
    """A compressed key whose x has no y on the curve."""
    rng = random.Random(31)
    while True:
        x = rng.randrange(1, P)
        if not O.fp_is_square((x**3 + 4) % P):
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80
            return bytes(b)


def off_curve_sig():
    rng = random.Random(32)
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        if not O.f2_is_square(O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.B_G2)):
            b = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
            b[0] |= 0x80
            return bytes(b)


@functools.lru_cache(maxsize=None)
def non_g1_key():
    from tests.test_gpu_kcoop import bad_keys

    return bad_keys()["rand non-G1"]


@functools.lru_cache(maxsize=None)
def non_g2_sig():
    from tests.test_gpu_kcoop import bad_sigs

    return bad_sigs()["rand non-G2"]


# ---- key stage -----------------------------------------------------------------
# One set: keys (48 bytes each), sks (the secret key of each, None for an
# invalid key), its randomizer and a tag naming the edge it stands for.
KeySet = namedtuple("KeySet", "keys sks r tag")
INVALID_KEYS = ("infinity key", "bad encoding", "off-curve x", "outside G1")
MULTI_SIZES = (2, 63, 64, 65, 130)


def invalid_key(tag):
    if tag == "infinity key":
        return O.INFINITY_G1
    if tag == "bad encoding":
        b = bytearray(pk_of(interop_sk(900)))
        b[0] &= 0x7F  # the compression flag cleared
        return bytes(b)
    if tag == "off-curve x":
        return off_curve_key()
    assert tag == "outside G1"
    return non_g1_key()


def key_sets():
    """About 100 sets: every edge randomizer and three dozen seeded ones on
    single keys, the four invalid keys, then the multi-key sets.  Not a
    multiple of 4 (k_keys_coop's rows) nor of 64 (a partial last block)."""
    sets = []
    nsk = [0]

    def fresh():
        nsk[0] += 1
        return interop_sk(1000 + nsk[0])

    def single(r, tag):
        sk = fresh()
        sets.append(KeySet([pk_of(sk)], [sk], r, tag))

    for r in edge_rands():
        single(r, "edge r")
    for r in seeded_rands(41, 36):
        single(r, "random r")
    for tag in INVALID_KEYS:
        sets.append(KeySet([invalid_key(tag)], [None], 0x0123456789ABCDEF, tag))
    mr = iter([M64, 0x0100000000000001, 1, 0x5555555555555555, 0xF0F0F0F00F0F0F0F] + seeded_rands(42, 8))
    for k in MULTI_SIZES:
        sks = [fresh() for _ in range(k)]
        sets.append(KeySet([pk_of(s) for s in sks], sks, next(mr), f"multi {k}"))
    a, b = fresh(), fresh()
    sets.append(KeySet([pk_of(a), pk_of(a)], [a, a], next(mr), "P, P"))
    sets.append(KeySet([pk_of(a), pk_of(-a)], [a, O.R - a], next(mr), "P, -P"))
    sets.append(KeySet([pk_of(a), pk_of(-a), pk_of(b)], [a, O.R - a, b], next(mr), "P, -P, Q"))
    sks = [fresh() for _ in range(5)]
    keys = [pk_of(s) for s in sks]
    keys[3] = invalid_key("outside G1")
    sks[3] = None
    sets.append(KeySet(keys, sks, next(mr), "multi with an invalid member"))
    return sets


KeyBatch = namedtuple("KeyBatch", "blob n_keys pk_off key_idx tab_n rands tags")


def key_batch(sets):
    """The byte form: the sets' keys in order."""
    off = [0]
    for s in sets:
        off.append(off[-1] + len(s.keys))
    return KeyBatch(b"".join(k for s in sets for k in s.keys), off[-1], off, None, 0, [s.r for s in sets], [s.tag for s in sets])


def key_batch_table(sets):
    """The table form: the same keys, once, as a table in reversed order,
    addressed through key_idx; two more sets carry an index >= tab_n (a
    single-key set at exactly tab_n, and one member of a three-key set)."""
    flat = [k for s in sets for k in s.keys]
    tab_n = len(flat)
    idx = [tab_n - 1 - j for j in range(tab_n)]
    off = [0]
    for s in sets:
        off.append(off[-1] + len(s.keys))
    idx += [tab_n]
    off.append(len(idx))
    idx += [tab_n - 1, tab_n + 5, tab_n - 2]
    off.append(len(idx))
    rands = [s.r for s in sets] + [3, 0x8000000000000001]
    tags = [s.tag for s in sets] + ["index == tab_n", "member index past the table"]
    return KeyBatch(b"".join(reversed(flat)), tab_n, off, idx, tab_n, rands, tags)


_G1J = O.jac_from_affine(O.FP, O.G1_GEN)


def neg_r_g1(r):
    x, y = O.jac_to_affine(O.FP, O.jac_mul(O.FP, _G1J, r))
    return (x, (-y) % P)


def key_reference(batch, unit_r=False):
    """Per set (P, P2, code) as stage_set_pk defines them: P = affine([r] sum
    of the keys) ((0, 0) with a code), P2 = affine(-[r] g1); unit_r: P = the sum."""
    keys = [batch.blob[48 * k : 48 * k + 48] for k in range(batch.n_keys)]
    decoded = {}
    out = []
    for i, r in enumerate(batch.rands):
        code, acc = O.SUCCESS, O.jac_inf(O.FP)
        for j in range(batch.pk_off[i], batch.pk_off[i + 1]):
            k = batch.key_idx[j] if batch.key_idx is not None else j
            if batch.key_idx is not None and k >= batch.tab_n:
                code = O.BAD_ENCODING
                break
            if k not in decoded:
                decoded[k] = O.pk_decode_validate(keys[k])
            kc, a = decoded[k]
            if kc != O.SUCCESS:
                code = O.PK_IS_INFINITY
                break
            acc = O.jac_add(O.FP, acc, O.jac_from_affine(O.FP, a))
        pt = None
        if code == O.SUCCESS:
            pt = O.jac_to_affine(O.FP, acc if unit_r else O.jac_mul(O.FP, acc, r))
            if pt is None:
                code = O.PK_IS_INFINITY
        out.append((pt or ZERO_G1, neg_r_g1(r), code))
    return out


# ---- signature checks ----------------------------------------------------------
def check_sigs():
    """70 signatures (not a multiple of 4 nor of 64): valid ones with, every
    few rows, the infinite signature, the bad encodings, an off-curve x and a
    point outside G2 -- in each row of k_sig_check_coop's four."""
    sigs = [sig_of(interop_sk(2000 + i)) for i in range(70)]
    flagless = bytearray(sigs[0])
    flagless[0] &= 0x7F
    inf_extra = bytearray(O.INFINITY_G2)
    inf_extra[95] = 1
    big_x = bytearray(b"\xff" * 96)
    big_x[0] = 0x9F  # compressed, x1 = 2^381 - 1 >= p
    bad = [O.INFINITY_G2, bytes(flagless), bytes(inf_extra), bytes(big_x), off_curve_sig(), non_g2_sig(), O.INFINITY_G2, non_g2_sig()]
    for k, b in enumerate(bad):
        sigs[8 * k + 1 + (k % 4)] = b  # rows 1, 2, 3, 0, ... of their workgroups
    sigs[69] = non_g2_sig()  # the last, in a partial workgroup and block
    return sigs


_sig_ref = {}


def sig_reference(sigs):
    """Per signature (Q, skip, code): Q the decoded point ((0, 0) without a
    pair), skip = 1 for an infinite or invalid signature, code from
    g2_decompress plus the subgroup test (infinity: 0)."""
    out = []
    for b in sigs:
        if b not in _sig_ref:
            code, a = O.sig_decode_validate(b)
            use = code == O.SUCCESS and a is not None
            _sig_ref[b] = (a if use else ZERO_G2, 0 if use else 1, code)
        out.append(_sig_ref[b])
    return out


# ---- bucket sums ---------------------------------------------------------------
# One batch: sigs (96 bytes each), sks (None for the infinite and the invalid
# signature), randomizers.
MsmCase = namedtuple("MsmCase", "name sigs sks rands")
SHARED_DIGIT_SIZES = (1, 31, 32, 33, 64, 65)  # around k_msm_bucket_tree's 32 lanes
REPEAT_SIZES = (2, 3, 32, 64)


def msm_cases():
    nsk = [0]

    def fresh():
        nsk[0] += 1
        return interop_sk(3000 + nsk[0])

    def case(name, sks, rands):
        sigs = [sig_of(s) for s in sks]
        return MsmCase(name, sigs, list(sks), list(rands))

    cases = [case("one set, r = 1", [fresh()], [1]), case("33 sets, r = 2^64 - 1", [fresh() for _ in range(33)], [M64] * 33)]
    for n in SHARED_DIGIT_SIZES:  # byte 0 is 0x5A in every r; the other bytes vary (and some are 0)
        hi = seeded_rands(50 + n, n)
        cases.append(case(f"{n} sets share a byte-0 digit", [fresh() for _ in range(n)], [0x5A | (h & ~0xFF & ~(0xFF << 24)) for h in hi]))
    a, b = fresh(), fresh()
    for n in REPEAT_SIZES:  # doubling in a lane's mixed addition (n > 32) and at every tree level
        cases.append(case(f"one signature {n} times, one r", [a] * n, [0x8000000000000301] * n))
    cases.append(case("A, -A, one r", [a, O.R - a], [0xC3] * 2))
    cases.append(case("A, -A, B, one r", [a, O.R - a, b], [0xC3] * 3))
    cases.append(case("A r = 1, -A r = 3", [a, O.R - a], [1, 3]))
    # the infinite and the outside-G2 signature in buckets the valid ones use
    sks = [fresh() for _ in range(6)]
    c = case("infinite and invalid signatures in used buckets", sks, [0x1107] * 6)
    c.sigs[2], c.sks[2] = O.INFINITY_G2, None
    c.sigs[4], c.sks[4] = non_g2_sig(), None
    cases.append(c)
    er = edge_rands()
    cases.append(case("edge randomizers (zero bytes)", [fresh() for _ in er], er))
    cases.append(case("300 sets, seeded r", [fresh() for _ in range(300)], seeded_rands(60, 300)))
    return cases


_NEG_POW2_G1 = []


def neg_pow2_g1():
    """-[2^j] g1, j < 64."""
    if not _NEG_POW2_G1:
        p = _G1J
        for _ in range(64):
            x, y = O.jac_to_affine(O.FP, p)
            _NEG_POW2_G1.append((x, (-y) % P))
            p = O.jac_double(O.FP, p)
    return _NEG_POW2_G1


def msm_reference(case):
    """(pairs, codes, n_bad, total): pairs[j] = (P_j, Q_j, skip_j) for j = 8w + k
    with Q_j = affine(sum of the valid finite sig_i whose r_i has bit j set),
    (0, 0) and skip 1 when that is infinity; total = the non-zero randomizer
    bytes over all sets."""
    ref = sig_reference(case.sigs)
    acc = [O.jac_inf(O.FP2) for _ in range(64)]
    for (q, skip, _), r in zip(ref, case.rands):
        if skip:
            continue
        qj = O.jac_from_affine(O.FP2, q)
        for j in range(64):
            if (r >> j) & 1:
                acc[j] = O.jac_add(O.FP2, acc[j], qj)
    pairs = []
    for j in range(64):
        a = O.jac_to_affine(O.FP2, acc[j])
        pairs.append((neg_pow2_g1()[j], a or ZERO_G2, 0 if a else 1))
    codes = [c for _, _, c in ref]
    total = sum(1 for r in case.rands for w in range(8) if (r >> (8 * w)) & 0xFF)
    return pairs, codes, sum(1 for c in codes if c), total


def bucket_reference(case):
    """{(w, d): affine sum or None} of the non-empty buckets, to name the
    bucket a failing pair comes from."""
    ref = sig_reference(case.sigs)
    out = {}
    for (q, skip, _), r in zip(ref, case.rands):
        for w in range(8):
            d = (r >> (8 * w)) & 0xFF
            if d:
                out.setdefault((w, d), O.jac_inf(O.FP2))
                if not skip:
                    out[(w, d)] = O.jac_add(O.FP2, out[(w, d)], O.jac_from_affine(O.FP2, q))
    return {k: O.jac_to_affine(O.FP2, v) for k, v in out.items()}


# ---- hash with a randomizer ----------------------------------------------------
def hash_rand_cases():
    """(msgs, rands): every edge randomizer and a dozen seeded ones, over
    messages of the lengths the hash kernel's paths split at."""
    rands = edge_rands() + seeded_rands(70, 12)
    rng = random.Random(71)
    lens = [0, 1, 31, 32, 33, 55, 56, 64, 119, 200, 768]
    msgs = [bytes(rng.getrandbits(8) for _ in range(lens[i % len(lens)])) for i in range(len(rands))]
    return msgs, rands


def hash_rand_reference(msgs, rands):
    """Q_i = affine([r_i] H(m_i)): the oracle's hash, multiplied here."""
    out = []
    for m, r in zip(msgs, rands):
        h = O.jac_from_affine(O.FP2, g2_of_bytes(C.hash_to_g2(m)))
        out.append(O.jac_to_affine(O.FP2, O.jac_mul(O.FP2, h, r)))
    return out
