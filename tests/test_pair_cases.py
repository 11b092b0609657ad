"""The references and comparators of tests/pair_cases.py against
oracle/bls12_381.py alone, without a GPU: what tests/test_gpu_pair_stage.py
holds the Miller-stage kernels to is right on its own.

  * the reference lines multiplied out are O.miller_loop exactly;
  * the segmented accumulator plus the Horner combine equal the unsegmented
    accumulator for every segment count the product uses;
  * a valid set's two Miller values pair to 1, a forged set's do not;
  * the line comparator accepts a line scaled in Fp2 and rejects a swapped
    line and a single changed limb; the Fp2 comparator rejects a ratio with
    any coordinate outside Fp2 set;
  * the byte codecs invert each other and canonicalise weakly reduced limbs.
"""

import random

import pytest

from oracle import bls12_381 as O
from tests import pair_cases as C

NSEGS = (1, 2, 3, 4, 5, 16)


@pytest.fixture(scope="module")
def pairs():
    return C.real_pairs(7)  # three [a] g1 / [b] g2 pairs and the four on hashed points


def test_step_kinds():
    assert C.STEP_KINDS.count("add") == 5 and C.STEP_KINDS[0] == "dbl" and C.STEP_KINDS[-1] == "dbl"
    assert [C.seg_bounds(j, 3) for j in range(3)] == [(0, 22), (22, 45), (45, 68)]
    assert sum(C.doublings_in(*C.seg_bounds(j, 16)) for j in range(16)) == 63


def test_reference_lines_multiply_out_to_miller_loop(pairs):
    for Pt, Qt, _ in (pairs[0], pairs[2], pairs[3], pairs[6]):
        lines = C.ref_lines(Pt, Qt)
        assert len(lines) == C.STEPS
        assert O.f12_conj(C.ref_segment([lines], 0, C.STEPS)) == O.miller_loop(Pt, Qt)
        assert C.ref_acc([lines], [True], [[0]], 1) == [[O.miller_loop(Pt, Qt)]]


def test_two_pairs_share_one_accumulator(pairs):
    """A group's value is the product of its valid pairs' Miller values; a
    killed pair contributes nothing, a group without valid pairs is exactly 1."""
    tabs = [C.ref_lines(Pt, Qt) for Pt, Qt, _ in pairs[:3]]
    want = O.f12_mul(O.miller_loop(*pairs[0][:2]), O.miller_loop(*pairs[2][:2]))
    assert C.ref_acc(tabs, [True, False, True], [[0, 1, 2]], 1)[0][0] == want
    assert C.ref_acc(tabs, [False] * 3, [[0, 1, 2]], 4) == [[O.F12_ONE]] * 4


def test_segments_recombine():
    tabs = C.random_lines(5, seed=7)
    groups = [[0, 2, 4], [1, 3]]
    valid = [True, True, False, True, True]
    whole = C.ref_acc(tabs, valid, groups, 1)[0]
    for nseg in NSEGS:
        segs = C.ref_acc(tabs, valid, groups, nseg)
        assert len(segs) == nseg
        for g in range(len(groups)):
            vals = [segs[j][g] for j in range(nseg)]
            assert C.ref_combine(vals) == whole[g], (nseg, g)
            assert C.ref_unsegmented(vals) == whole[g], (nseg, g)


def test_group_layouts_cover_every_pair_once():
    for n, per in ((133, 1), (133, 2), (133, 8), (133, 32), (74, 2), (5, 8)):
        for groups in (C.groups_contiguous(n, per), C.groups_strided(n, per)):
            assert sorted(i for own in groups for i in own) == list(range(n))
            assert len(groups) == (n + per - 1) // per and all(0 < len(own) <= per for own in groups)
    assert C.groups_strided(74, 2)[5] == [5, 42]  # the settle shape: thread g owns g and g + n
    assert C.groups_contiguous(133, 2)[-1] == [132]


def test_kill_flags_cover_the_accumulator_paths():
    for n, per in ((133, 4), (133, 8), (133, 32)):
        groups = C.groups_strided(n, per)
        valid = C.valid_of(C.kill_flags(n, groups, seed=3))
        counts = [sum(valid[i] for i in own) for own in groups[:5]]
        assert counts == [0, 1, 2, 3, len(groups[4])], (n, per)
    valid = C.valid_of(C.kill_flags(133, C.groups_strided(133, 2), seed=3))
    killed = 133 - sum(valid)
    assert 15 < killed < 60  # about a quarter
    for arr in C.kill_flags(133, C.groups_strided(133, 2), seed=3):
        assert any(arr)  # each of the three flag arrays kills some pair


def test_valid_set_pairs_to_one_forged_does_not():
    Ps, Qs = C.settle_sets(2, forged={1})
    for g, want in ((0, True), (1, False)):
        v = O.f12_mul(O.miller_loop(Ps[g], Qs[g]), O.miller_loop(Ps[2 + g], Qs[2 + g]))
        assert (O.final_exponentiation(v) == O.F12_ONE) is want


def test_product_of_known_pairs_is_a_power_of_the_generator_pairing(pairs):
    f = C.ref_product([O.miller_loop(Pt, Qt) for Pt, Qt, _ in pairs])  # the hashed pairs cancel: (g1, H) (-g1, H)
    e = sum(e for _, _, e in pairs if e is not None)
    assert O.final_exponentiation(f) == O.f12_pow(O.pairing(O.G1_GEN, O.G2_GEN), e)


# ---- comparators -------------------------------------------------------------------------
def test_line_comparator(pairs):
    rng = random.Random(11)
    lines = C.ref_lines(*pairs[0][:2])
    for s in (0, 1, 17, 67):
        a, b, c = lines[s]
        k = C.random_fp2(rng)
        assert not O.f2_is_zero(k)
        scaled = (O.f2_mul(a, k), O.f2_mul(b, k), O.f2_mul(c, k))
        assert C.line_matches(scaled, lines[s])
        assert not C.line_matches((scaled[1], scaled[0], scaled[2]), lines[s])  # a and b swapped
        assert not C.line_matches((O.F2_ZERO,) * 3, lines[s])
        assert not C.line_matches(None, lines[s])
    # one limb changed in the encoded table
    scaled = [[tuple(O.f2_mul(x, (3, 5)) for x in ln) for ln in lines]]
    raw = bytearray(C.enc_line_table(scaled))
    assert C.line_mismatch(C.dec_line_table(bytes(raw), 1)[0], lines) is None
    word = (40 * C.LINE_G + 7) * 16  # step 40, group 7: limbs 4 .. 7 of b.c0
    raw[word + 4] ^= 1
    assert C.line_mismatch(C.dec_line_table(bytes(raw), 1)[0], lines) == (40, "ab")


def test_fp2_comparator(pairs):
    f = O.miller_loop(*pairs[0][:2])
    k = (((7, O.P - 3), O.F2_ZERO, O.F2_ZERO), O.F6_ZERO)  # an Fp2 element
    assert C.same_up_to_fp2(O.f12_mul(f, k), f) and C.same_up_to_fp2(f, f)
    assert C.ratio_defect([0, 0] + [0] * 10) == 0  # the Fp2 coefficient itself must not vanish
    assert C.ratio_defect([0, 5] + [0] * 10) is None
    for c in range(2, 12):  # any higher coordinate set
        flat = [7, 9] + [0] * 10
        flat[c] = 1
        assert C.ratio_defect(flat) == c
        assert not C.same_up_to_fp2(O.f12_mul(f, C.f12_unflat(flat)), f)
    assert not C.same_up_to_fp2(O.f12_sqr(f), f)


# ---- codecs ----------------------------------------------------------------------------------
def test_codecs_round_trip_and_canonicalise():
    rng = random.Random(13)
    for v in (0, 1, O.P - 1, rng.randrange(O.P)):
        assert C.dec_fp(C.enc_fp(v)) == v
        weak = int.from_bytes(C.enc_fp(v), "little") + O.P  # the same element, weakly reduced
        assert C.dec_fp(weak.to_bytes(48, "little")) == v
    f = C.random_f12(rng)
    assert C.dec_f12(C.enc_f12(f)) == f and len(C.enc_f12(f)) == C.F12_BYTES
    assert C.dec_f12s(C.enc_f12(f) + b"\xee" * 576, 2) == [f, None]
    assert C.dec_f12(C.enc_f12(O.F12_ONE)) == O.F12_ONE
    tabs = C.random_lines(3, seed=5)
    raw = C.enc_line_table([tabs[0], None, tabs[2]])
    assert len(raw) == C.STEPS * C.LINE_G * 3 * 16
    back = C.dec_line_table(raw, 3)
    assert back[0] == tabs[0] and back[2] == tabs[2] and back[1] == [None] * C.STEPS
    pt = C.g1_mul(5)
    assert C.dec_g1(C.enc_g1(pt)) == pt and C.dec_g2(C.enc_g2(O.G2_GEN)) == O.G2_GEN
