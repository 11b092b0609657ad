"""Sync-committee verification from the device-resident key table: by key
index (tbls_fast_aggregate_verify_many_idx) and by a resident committee plus a
participation bitvector (tbls_committee_load /
tbls_fast_aggregate_verify_many_bits, k_set_pk_bits_coop).

Every verdict is compared with the C oracle's fastAggregateVerify
(oracle/c/bls_oracle.c, BLS.java:185-207) on the participants' key bytes in
committee order.  A set is signed once with the sum of its participants'
secret keys (as tests/test_gpu_configs.py::test_multi_key_exceptional_sums),
which is the aggregate of their individual signatures.  Shapes are small: the
cooperative rows hold one or two members at committee size 40, and 512 is the
real committee.
"""

import os
import random
import subprocess
import sys

import pytest

from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, os.cpu_count() or 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_PLAIN = 600  # table: interop keys [0, 600), then the invalid keys, then negations
I_INF, I_BAD, I_NEG = 600, 601, 602
N_NEG = 24  # table[I_NEG + i] = -table[i]


@pytest.fixture(scope="module")
def W():
    """The module's world: synth, bls and the big table's keys (bytes) and
    secret keys (None for the two invalid keys), computed once."""
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import bls, native, synth

    native.lib()
    R = synth.R_ORDER
    sks = [synth.interop_sk(60000 + i) for i in range(N_PLAIN)]
    neg = [R - sks[i] for i in range(N_NEG)]
    pks = synth.pubkeys(sks + neg)

    class World:
        pass

    w = World()
    w.S, w.bls, w.native, w.R = synth, bls, native, R
    w.sk = sks + [None, None] + neg
    w.pk = pks[:N_PLAIN] + [synth.INFINITY_G1, synth.BAD_PK] + pks[N_PLAIN:]
    return w


@pytest.fixture
def T(W):
    """The big table, loaded afresh (every committee slot empty)."""
    t = W.bls.ValidatorKeyTable(W.pk)
    assert t.codes[:N_PLAIN] == [0] * N_PLAIN and t.codes[I_INF] != 0 and t.codes[I_BAD] != 0
    assert t.codes[I_NEG:] == [0] * N_NEG
    return t


def _bits(pattern):
    out = bytearray((len(pattern) + 7) // 8)
    for i, p in enumerate(pattern):
        if p:
            out[i // 8] |= 1 << (i % 8)
    return bytes(out)


def _pick(size, count, seed):
    """A participation pattern of `count` members of `size`, from a fixed seed."""
    chosen = set(random.Random(seed).sample(range(size), count))
    return [i in chosen for i in range(size)]


def _build(W, members, patterns, seed):
    """Sets over committee `members` (table indices) for the given patterns:
    (bits, msgs, sigs, key lists).  Each set is signed with the sum of its
    participants' secret keys (invalid members add nothing; a zero sum gets
    the infinity signature, the only one that could pair with it)."""
    msgs = [W.S.bench_message(seed, s) for s in range(len(patterns))]
    agg = []
    keys = []
    for pat in patterns:
        assert len(pat) == len(members)
        part = [m for m, p in zip(members, pat) if p]
        agg.append(sum(W.sk[m] for m in part if W.sk[m] is not None) % W.R)
        keys.append([W.pk[m] for m in part])
    blob = W.S.sign_blob([a if a else 1 for a in agg], msgs)
    sigs = [blob[96 * s : 96 * s + 96] if agg[s] else W.S.INFINITY_G2 for s in range(len(patterns))]
    return [_bits(p) for p in patterns], msgs, sigs, keys


def _check(W, committee, bits, msgs, sigs, keys, expect=None):
    got = committee.fast_aggregate_verify_many(list(zip(bits, msgs, sigs)))
    exp = C.verify_each(keys, msgs, sigs, threads=THREADS)
    assert got == exp, (got, exp)
    if expect is not None:
        assert got == expect, (got, expect)
    return got


# ---------------------------------------------------------------------------
def test_by_index(W):
    """tbls_fast_aggregate_verify_many_idx: a table of 48 interop keys, the
    infinity key and BAD_PK; sets of 1, 2, 33 and 40 keys.  Verdicts equal the
    by-bytes call and the oracle: all valid (the randomized batch accepts), and
    with a tampered signature, a key swapped for a non-signer, a set naming
    each invalid key and an empty set (the per-set pass)."""
    S = W.S
    tab_pk = W.pk[:48] + [S.INFINITY_G1, S.BAD_PK]
    table = W.bls.ValidatorKeyTable(tab_pk)
    assert table.size == 50
    rng = random.Random(11)
    idx = [rng.sample(range(47), k) for k in (1, 2, 33, 40)]  # key 47 signs nothing
    msgs = [S.bench_message(31, s) for s in range(9)]
    agg = [sum(W.sk[k] for k in ks) % W.R for ks in idx]
    blob = S.sign_blob(agg, msgs[:4])
    sigs = [blob[96 * s : 96 * s + 96] for s in range(4)]

    def run(idx_sets, m, s):
        got = table.fast_aggregate_verify_many(list(zip(idx_sets, m, s)))
        keys = [[tab_pk[k] for k in ks] for ks in idx_sets]
        assert got == S.SetArray.from_lists(keys, m, s).fast_aggregate_verify_many()
        assert got == C.verify_each(keys, m, s, threads=THREADS)
        return got

    assert run(idx, msgs[:4], sigs) == [True] * 4
    swapped = list(idx[3])
    swapped[17] = 47
    more_idx = idx + [idx[2], swapped, idx[1] + [48], [idx[0][0], 49], []]
    more_msgs = msgs[:4] + [msgs[2], msgs[3], msgs[1], msgs[0], msgs[8]]
    more_sigs = sigs + [sigs[3], sigs[3], sigs[1], sigs[0], sigs[0]]
    assert run(more_idx, more_msgs, more_sigs) == [True] * 4 + [False] * 5
    assert run([[]], [msgs[0]], [sigs[0]]) == [False]
    with pytest.raises(ValueError):
        table.fast_aggregate_verify_many([([50], msgs[0], sigs[0])])
    with pytest.raises(ValueError):
        table.fast_aggregate_verify_many([(idx[1], msgs[1], sigs[1]), ([3, 2**32 - 1], msgs[0], sigs[0])])


_NO_TABLE = """
import ctypes, sys
import torch  # noqa: F401
from teku_amd import native
L = native.lib()
assert L.tbls_pk_table_size() == 0
idx = (ctypes.c_uint32 * 1)(0)
msg, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(bytes([0xC0]) + bytes(95), 96)
s = (native.TblsSetIdx * 1)()
s[0].key_idx, s[0].n_pks = ctypes.cast(idx, ctypes.c_void_p), 1
s[0].msg, s[0].msg_len, s[0].sig = ctypes.cast(msg, ctypes.c_void_p), 32, ctypes.cast(sig, ctypes.c_void_p)
out = (ctypes.c_int * 1)()
rc = [L.tbls_fast_aggregate_verify_many_idx(s, 1, out), L.tbls_committee_load(0, idx, 1), L.tbls_committee_size(0)]
b = (native.TblsSetBits * 1)()
b[0].bits, b[0].msg, b[0].msg_len, b[0].sig = s[0].key_idx, s[0].msg, 32, s[0].sig
rc.append(L.tbls_fast_aggregate_verify_many_bits(0, b, 1, out))
print("RC", rc)
from teku_amd import bls
t = object.__new__(bls.ValidatorKeyTable)  # the wrapper without a load
try:
    t.fast_aggregate_verify_many([([0], bytes(32), bytes([0xC0]) + bytes(95))])
    raised = False
except ValueError:
    raised = True
print("RAISED", raised)
sys.exit(0 if raised and rc == [native.BAD_ARGUMENT, native.BAD_ARGUMENT, 0, native.BAD_ARGUMENT] else 1)
"""


def test_no_table_is_bad_argument(W):
    """A process that never loaded a table (a fresh one: the table is process
    state and cannot be unloaded): the index call, the committee load and the
    bitfield call all give TBLS_BAD_ARGUMENT, which the wrappers raise as
    ValueError."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NO_TABLE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_side_choice_boundary(W, T):
    """Committee of 40 (rows hold one or two members): participation 40, 39,
    21 (complement: fewer absent than present), 20 (tie: direct), 19, 1, 0;
    for 39 also a signer's bit cleared and the non-signer's bit set; one
    tampered signature."""
    members = list(range(100, 140))
    com = T.load_committee(0, members)
    assert com.size == 40 and W.native.lib().tbls_committee_size(0) == 40
    counts = [40, 39, 21, 20, 19, 1, 0]
    pats = [_pick(40, c, 500 + c) for c in counts]
    bits, msgs, sigs, keys = _build(W, members, pats, seed=41)
    valid = [i for i, c in enumerate(counts) if c]
    # all valid: the randomized batch accepts
    sel = lambda xs: [xs[i] for i in valid]  # noqa: E731
    _check(W, com, sel(bits), sel(msgs), sel(sigs), sel(keys), [True] * len(valid))
    # the whole list, with the tampers: the per-set pass
    p39 = pats[1]
    absent = p39.index(False)
    signer = p39.index(True)
    cleared = list(p39)
    cleared[signer] = False
    added = list(p39)
    added[absent] = True
    xb = bits + [_bits(cleared), _bits(added), bits[0]]
    xm = msgs + [msgs[1], msgs[1], msgs[0]]
    xs = sigs + [sigs[1], sigs[1], sigs[2]]
    xk = keys + [[W.pk[m] for m, p in zip(members, cleared) if p], [W.pk[m] for m, p in zip(members, added) if p], keys[0]]
    _check(W, com, xb, xm, xs, xk, [True] * 6 + [False] * 4)


@pytest.mark.parametrize("size", [1, 31, 32, 33, 512])
def test_committee_size_edges(W, T, size):
    """Sizes around one word of the bit row and the real committee: four sets
    with everyone participating, four with all but three."""
    members = [(7 * i + 3) % N_PLAIN for i in range(size)] if size < 512 else list(range(40, 552))
    com = T.load_committee(1, members)
    pats = [[True] * size for _ in range(4)] + [_pick(size, max(0, size - 3), 900 + 10 * size + s) for s in range(4)]
    bits, msgs, sigs, keys = _build(W, members, pats, seed=1000 + size)
    _check(W, com, bits, msgs, sigs, keys, [True] * 4 + [size > 3] * 4)


def test_invalid_members(W, T):
    """The infinity key and BAD_PK as members: absent they do not matter (few
    participants: direct side; every valid member: complement side); a set in
    which one participates fails."""
    members = list(range(200, 220)) + [I_INF] + list(range(220, 238)) + [I_BAD]
    com = T.load_committee(2, members)
    n = len(members)
    few = [i in (3, 17, 30) for i in range(n)]
    most = [i not in (20, 39) for i in range(n)]
    few_inf = [i in (3, 17, 20) for i in range(n)]
    most_bad = [i != 20 for i in range(n)]
    most_inf = [i != 39 for i in range(n)]
    bits, msgs, sigs, keys = _build(W, members, [few, most, few_inf, most_bad, most_inf], seed=43)
    _check(W, com, bits[:2], msgs[:2], sigs[:2], keys[:2], [True, True])
    _check(W, com, bits, msgs, sigs, keys, [True, True, False, False, False])


@pytest.mark.parametrize("dup", [32, 1], ids=["same_row", "other_row"])
def test_duplicate_members(W, T, dup):
    """The same validator at positions 0 and `dup`: both present (all members,
    and three members on the direct side), one present, both absent under
    near-full participation (the same key subtracted twice)."""
    members = list(range(300, 340))
    members[dup] = members[0]
    com = T.load_committee(0, members)
    full = [True] * 40
    three = [i in (0, dup, 9) for i in range(40)]
    one = [i != dup for i in range(40)]
    none = [i not in (0, dup) for i in range(40)]
    bits, msgs, sigs, keys = _build(W, members, [full, three, one, none], seed=44 + dup)
    _check(W, com, bits, msgs, sigs, keys, [True] * 4)
    # a signature over the set without the repeat must not pass as the set with it
    _check(W, com, [bits[0]], [msgs[2]], [sigs[2]], [keys[0]], [False])


def test_cancelling_members(W, T):
    """A key beside its negation; a committee whose sum is infinity (no usable
    committee sum: the direct side answers); [k, -k, a] with the first two
    participating (the complement meets a - a)."""
    inf_sig = W.S.INFINITY_G2
    members = list(range(40))
    members[7] = I_NEG + 3  # -key 3, rows 7 and 3
    members[35] = I_NEG + 3  # and again, in row 3 beside key 3
    com = T.load_committee(0, members)
    full = [True] * 40
    absent = [i not in (3, 7, 35) for i in range(40)]
    pair = [i in (3, 35) for i in range(40)]
    bits, msgs, sigs, keys = _build(W, members, [full, absent, pair], seed=46)
    assert sigs[2] == inf_sig
    _check(W, com, bits, msgs, sigs, keys, [True, True, False])

    members = []
    for k in range(10):
        members += [k, I_NEG + k]
    com = T.load_committee(1, members)
    pats = [[True] * 20, [i != 4 for i in range(20)], [i not in (5, 12) for i in range(20)], [i in (0, 1) for i in range(20)]]
    bits, msgs, sigs, keys = _build(W, members, pats, seed=47)
    assert sigs[0] == inf_sig and sigs[3] == inf_sig
    _check(W, com, bits, msgs, sigs, keys, [False, True, True, False])
    _check(W, com, bits[1:3], msgs[1:3], sigs[1:3], keys[1:3], [True, True])

    members = [5, I_NEG + 5, 77]
    com = T.load_committee(2, members)
    bits, msgs, sigs, keys = _build(W, members, [[True, True, False], [True, True, True]], seed=48)
    assert sigs[0] == inf_sig
    _check(W, com, bits, msgs, sigs, keys, [False, True])


def test_state_and_arguments(W, T):
    """Reloading a slot replaces it; loading a table empties the slots; the
    argument errors of the load and of the bitfield call."""
    a, b = list(range(400, 433)), list(range(433, 466))
    com = T.load_committee(3, a)
    pat = _pick(33, 30, 5)
    bits_a, msgs, sigs_a, keys_a = _build(W, a, [pat], seed=49)
    _, _, sigs_b, keys_b = _build(W, b, [pat], seed=49)
    _check(W, com, bits_a, msgs, sigs_a, keys_a, [True])
    com = T.load_committee(3, b)
    _check(W, com, bits_a, msgs, sigs_a, keys_b, [False])
    _check(W, com, bits_a, msgs, sigs_b, keys_b, [True])
    past = bytearray(bits_a[0])
    past[4] |= 0x02  # bit 33 of a committee of 33
    with pytest.raises(ValueError):
        com.fast_aggregate_verify_many([(bytes(past), msgs[0], sigs_b[0])])
    for slot, idx in [(4, a), (0, []), (0, [1] * 2049), (0, [0, len(W.pk)]), (2**32, a)]:
        with pytest.raises(ValueError):
            T.load_committee(slot, idx)
    L = W.native.lib()
    assert [L.tbls_committee_size(s) for s in range(5)] == [0, 0, 0, 33, 0]
    assert T.load_committee(0, [1] * 2048).size == 2048
    W.bls.ValidatorKeyTable(W.pk)  # the same keys: the slots are emptied all the same
    assert [L.tbls_committee_size(s) for s in range(4)] == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        com.fast_aggregate_verify_many([(bits_a[0], msgs[0], sigs_b[0])])


def test_batch_and_per_set_paths(W, T):
    """Eight valid sets (the randomized batch settles them), then the same
    call with one bad set (the per-set pass gives the verdicts)."""
    members = list(range(450, 490))
    com = T.load_committee(0, members)
    pats = [_pick(40, c, 70 + c) for c in (40, 38, 37, 30, 12, 5, 2, 1)]
    bits, msgs, sigs, keys = _build(W, members, pats, seed=50)
    _check(W, com, bits, msgs, sigs, keys, [True] * 8)
    sigs[6] = sigs[5]
    _check(W, com, bits, msgs, sigs, keys, [True] * 6 + [False, True])


def test_config2_small(W, T):
    """Config 2 in small: 8 sets over one 512-member committee, 507
    participants each; then three tampers as tests/test_gpu_configs.py's config
    2 -- a signature over another message, a key swapped for a non-signer, the
    infinity key.  The by-index call on the same participants agrees."""
    members = list(range(30, 541)) + [I_INF]  # 511 valid members and the infinity key, absent below
    com = T.load_committee(1, members)
    pats = []
    for s in range(8):
        chosen = set(random.Random(2000 + s).sample(range(511), 507))
        pats.append([i in chosen for i in range(512)])
    bits, msgs, sigs, keys = _build(W, members, pats, seed=2)
    _check(W, com, bits, msgs, sigs, keys, [True] * 8)
    by_idx = [[m for m, p in zip(members, pat) if p] for pat in pats]
    assert T.fast_aggregate_verify_many(list(zip(by_idx, msgs, sigs))) == [True] * 8
    p2, s2 = [list(p) for p in pats], list(sigs)
    s2[5] = sigs[6]
    out, inn = p2[2].index(False), p2[2].index(True)
    p2[2][out], p2[2][inn] = True, False
    p2[7][511] = True
    b2 = [_bits(p) for p in p2]
    k2 = [[W.pk[m] for m, p in zip(members, pat) if p] for pat in p2]
    got = _check(W, com, b2, msgs, s2, k2)
    assert [i for i, v in enumerate(got) if not v] == [2, 5, 7]
    idx2 = [[m for m, p in zip(members, pat) if p] for pat in p2]
    assert T.fast_aggregate_verify_many(list(zip(idx2, msgs, s2))) == got
