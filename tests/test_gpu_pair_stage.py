"""Byte-level parity of the Miller stage: lines, accumulators, products.

The stages before the Miller loop are compared with a plain reference at
their own outputs (tests/test_gpu_ops.py, test_gpu_hash_variants.py,
test_gpu_stages.py, test_gpu_pk*.py); this module does the same for the
kernels of the loop itself and of the settle paths, which the other tests
reach only through whole batches and their verdicts.  Through the test
library's hook (tests/native/k_test_pair.hip), which launches the PRODUCT
library's kernels with the grids and blocks of tb_lib.hip, these run on the
cases of tests/pair_cases.py and every output slot is compared:

  k_miller_lines_w2 / _quad / _duo, k_gsettle_msg_lines   the 68 lines per pair
  k_miller_acc1, k_miller_acc2, k_miller_accs_lds         every group and segment
  k_miller_accs_gsettle, k_gsettle_prep, k_settle_mask    the settle inputs and values
  k_fp12_prod_wave, k_fp12_prod_wave_seg                  every chunk product
  k_fp12_seg_combine_coop, k_group_test_coop              the Horner combine, the verdicts
  k_miller_wave                                           with its skip and code flags

There is no tolerance anywhere: the kernels are field arithmetic with exactly
determined results, and every number below is a shape, an index or a seed.
Values are compared as canonical integers mod p.  Two comparisons are exact
without being equalities (tests/pair_cases.py): a device line is projective,
the oracle's affine line times a nonzero Fp2 factor, and a Miller value built
from such lines equals the oracle's up to a nonzero Fp2 factor, which the
final exponentiation kills.  The three line kernels compute the same field
elements (tb_quad.h states it), so their tables are also compared with each
other for equality mod p.

Every output buffer comes back preset to 0xEE with a guard region behind it:
a slot the kernel must not write (a killed pair's lines, a padded lane, a
position outside the chunk) must still read 0xEE, and so must the guard.
TB_BLOCK is 64; the shapes are the smallest that span a full and a partial
block.  tests/test_pair_cases.py checks the references and comparators
against the oracle without a GPU.
"""

import ctypes
import functools
import random

import pytest

from oracle import bls12_381 as O
from tests import pair_cases as C

pytestmark = pytest.mark.gpu

LINE_KERNELS = {0: "k_miller_lines_w2", 1: "k_miller_lines_quad", 2: "k_miller_lines_duo"}
ACC_KERNELS = {0: "k_miller_acc1", 1: "k_miller_acc2", 2: "k_miller_accs_lds"}
EE = C.UNWRITTEN
NSEGS = (1, 2, 3, 4, 5, 16)


def _launched(rc, what):
    """A hook's negative code is a failed HIP call (a launch, a copy, the
    synchronize): nothing more may run on that device, so the session ends."""
    if rc:
        pytest.exit(f"tests/native/k_test_pair.hip: {what}: HIP call failed ({rc}); no further GPU work", returncode=3)


@pytest.fixture(scope="module")
def hook():
    from teku_amd import native
    from tests.opcodec import load_test_lib

    L = load_test_lib()
    vp, cp, ci, u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32
    L.tbls_test_pair_guard.restype = ctypes.c_size_t
    L.tbls_test_pair_guard.argtypes = []
    sigs = {
        "lines": [cp, ci, cp, cp, cp, cp, cp, u32, vp],
        "msg_lines": [cp, cp, cp, u32, vp],
        "acc": [cp, ci, cp, cp, cp, cp, u32, u32, u32, vp],
        "accs_gsettle": [cp, cp, u32, vp, vp, cp, cp, cp, cp, cp, cp, u32, u32, u32, u32, vp],
        "gsettle_prep": [cp, vp, vp, u32, u32, u32, u32, vp, cp, cp, cp, cp, cp, vp, vp, vp, vp],
        "prod": [cp, cp, u32, u32, u32, vp],
        "prod_seg": [cp, cp, u32, u32, u32, u32, u32, u32, u32, vp, u32],
        "combine": [cp, cp, u32, vp],
        "group_test": [cp, cp, u32, u32, vp, u32, vp],
        "miller_wave": [cp, cp, cp, cp, cp, cp, u32, vp],
        "settle_mask": [cp, cp, u32, vp],
    }
    for name, argtypes in sigs.items():
        fn = getattr(L, "tbls_test_pair_" + name)
        fn.restype, fn.argtypes = ci, argtypes
    so = native.LIB_PATH.encode()
    guard = L.tbls_test_pair_guard()

    def out(size):
        return ctypes.create_string_buffer(size + guard)

    def done(rc, what, *bufs):
        """The payloads of the output buffers, once the call and every guard are good."""
        assert rc != -1, (what, "shape refused by the hook before any launch")
        _launched(rc, what)
        res = []
        for b in bufs:
            raw = b.raw
            assert raw[len(raw) - guard :] == bytes([EE]) * guard, (what, "wrote into the guard behind an output")
            res.append(raw[: len(raw) - guard])
        return res[0] if len(res) == 1 else res

    def u32s(v):
        return (ctypes.c_uint32 * len(v))(*v)

    def u64s(v):
        return (ctypes.c_uint64 * len(v))(*v)

    def pts(enc, v):
        return b"".join(enc(x) for x in v)

    class Hook:
        @staticmethod
        def lines(variant, Ps, Qs, flags):
            n = len(Ps)
            o = out(C.STEPS * C.LINE_G * n * 16)
            rc = L.tbls_test_pair_lines(so, variant, pts(C.enc_g1, Ps), pts(C.enc_g2, Qs), *(bytes(f) for f in flags), n, o)
            return done(rc, LINE_KERNELS[variant], o)

        @staticmethod
        def msg_lines(Qs, skip):
            m = len(Qs)
            o = out(C.STEPS * C.LINE_G * m * 16)
            return done(L.tbls_test_pair_msg_lines(so, pts(C.enc_g2, Qs), bytes(skip), m, o), "k_gsettle_msg_lines", o)

        @staticmethod
        def acc(variant, table, flags, n, per, nseg):
            """[segment][group] values of f_out (seg_stride = G); None where unwritten."""
            G = (n + per - 1) // per
            o = out(nseg * G * C.F12_BYTES)
            rc = L.tbls_test_pair_acc(so, variant, table, *(bytes(f) for f in flags), n, per, nseg, o)
            raw = done(rc, f"{ACC_KERNELS[variant]} n={n} per={per} nseg={nseg}", o)
            vals = C.dec_f12s(raw, nseg * G)
            return raw, [vals[j * G : (j + 1) * G] for j in range(nseg)]

        @staticmethod
        def accs_gsettle(mlines, m, msg_of_pos, grp_sets, set_P, set_code, sig_code, msg_skip, slines, sskip, lo, cn, n, nseg):
            o = out(nseg * n * C.F12_BYTES)
            rc = L.tbls_test_pair_accs_gsettle(so, mlines, m, u32s(msg_of_pos), u32s(grp_sets), pts(C.enc_g1, set_P), bytes(set_code),
                                               bytes(sig_code), bytes(msg_skip), slines, bytes(sskip), lo, cn, n, nseg, o)
            return C.dec_f12s(done(rc, "k_miller_accs_gsettle", o), nseg * n)

        @staticmethod
        def gsettle_prep(grp_off, grp_sets, m, n, lo, cn, rands, sig_aff, sig_use, set_code, sig_code, msg_skip):
            o = [out(4 * n), out(96 * cn), out(192 * cn), out(cn)]
            rc = L.tbls_test_pair_gsettle_prep(so, u32s(grp_off), u32s(grp_sets), m, n, lo, cn, u64s(rands), sig_aff, bytes(sig_use),
                                               bytes(set_code), bytes(sig_code), bytes(msg_skip), *o)
            return done(rc, "k_gsettle_prep", *o)

        @staticmethod
        def prod(vals, n, chunk, grid):
            o = out(grid * C.F12_BYTES)
            rc = L.tbls_test_pair_prod(so, b"".join(C.enc_f12(v) for v in vals[:n]), n, chunk, grid, o)
            return C.dec_f12s(done(rc, f"k_fp12_prod_wave n={n} chunk={chunk} grid={grid}", o), grid)

        @staticmethod
        def prod_seg_raw(raw_in, in_count, n, n_last, nseg, in_stride, chunk, grid_x, out_stride):
            count = (nseg - 1) * out_stride + grid_x
            o = out(count * C.F12_BYTES)
            rc = L.tbls_test_pair_prod_seg(so, raw_in, in_count, n, n_last, nseg, in_stride, chunk, grid_x, o, out_stride)
            return done(rc, f"k_fp12_prod_wave_seg n={n} n_last={n_last} nseg={nseg} chunk={chunk}", o)

        @staticmethod
        def combine_raw(raw_in, nseg):
            o = out(C.F12_BYTES)
            return C.dec_f12(done(L.tbls_test_pair_combine(so, raw_in, nseg, o), f"k_fp12_seg_combine_coop nseg={nseg}", o))

        @staticmethod
        def group_test(raw_vals, stride, nseg, groups):
            o = out(len(groups))
            rc = L.tbls_test_pair_group_test(so, raw_vals, stride, nseg, u32s(groups), len(groups), o)
            return list(done(rc, f"k_group_test_coop stride={stride} nseg={nseg}", o))

        @staticmethod
        def miller_wave(Ps, Qs, flags):
            n = len(Ps)
            o = out(n * C.F12_BYTES)
            rc = L.tbls_test_pair_miller_wave(so, pts(C.enc_g1, Ps), pts(C.enc_g2, Qs), *(bytes(f) for f in flags), n, o)
            return C.dec_f12s(done(rc, "k_miller_wave", o), n)

        @staticmethod
        def settle_mask(set_code, n, skip):
            buf = ctypes.create_string_buffer(bytes(skip), 2 * n)
            rc = L.tbls_test_pair_settle_mask(so, bytes(set_code), n, buf)
            _launched(rc, "k_settle_mask")
            assert rc == 0
            return list(buf.raw)

    return Hook


# ---- real pairs: the line kernels and the chain ------------------------------------------------
N_REAL = 70
# killed: the first pair, pairs 63 and 64 (the block edge), the last pair, and one more per flag array
REAL_KILL = ({0: 1, 20: 1, 64: 0xFF}, {33: 2, 63: 1}, {47: 1, 69: 3})  # skip, code_a, code_b


class RealCase:
    def __init__(self):
        self.pairs = C.real_pairs(N_REAL)
        self.Ps = [p for p, _, _ in self.pairs]
        self.Qs = [q for _, q, _ in self.pairs]
        self.flags = tuple([kill.get(i, 0) for i in range(N_REAL)] for kill in REAL_KILL)
        self.valid = C.valid_of(self.flags)
        self.lines = [C.ref_lines(p, q) if v else None for (p, q, _), v in zip(self.pairs, self.valid)]

    @functools.cached_property
    def miller_product(self):
        """prod of O.miller_loop over the live pairs."""
        return C.ref_product([O.miller_loop(p, q) for (p, q, _), v in zip(self.pairs, self.valid) if v])

    @functools.cached_property
    def pairing(self):
        """The live pairs' pairing product from the known scalars: e(g1, g2)^(sum a b),
        times the pairings of the live pairs on hashed points."""
        want = O.f12_pow(O.pairing(O.G1_GEN, O.G2_GEN), sum(e for (_, _, e), v in zip(self.pairs, self.valid) if v and e is not None))
        for (p, q, e), v in zip(self.pairs, self.valid):
            if v and e is None:
                want = O.f12_mul(want, O.pairing(p, q))
        return want


@pytest.fixture(scope="module")
def real():
    case = RealCase()
    assert sorted(i for i, v in enumerate(case.valid) if not v) == [0, 20, 33, 47, 63, 64, 69]
    return case


@pytest.fixture(scope="module")
def line_tables(hook, real):
    """variant -> (raw table, decoded table), each kernel launched once."""
    cache = {}

    def get(variant):
        if variant not in cache:
            raw = hook.lines(variant, real.Ps, real.Qs, real.flags)
            cache[variant] = (raw, C.dec_line_table(raw, N_REAL))
        return cache[variant]

    return get


@pytest.mark.parametrize("variant", sorted(LINE_KERNELS), ids=[LINE_KERNELS[v] for v in sorted(LINE_KERNELS)])
def test_line_kernel(real, line_tables, variant):
    """70 pairs: every live pair's 68 lines match the reference projectively,
    every line slot of a killed pair is still 0xEE (the guard is checked by
    the hook wrapper)."""
    name = LINE_KERNELS[variant]
    _, dev = line_tables(variant)
    for i in range(N_REAL):
        if real.valid[i]:
            bad = C.line_mismatch(dev[i], real.lines[i])
            assert bad is None, f"{name} n={N_REAL}: pair {i}, step {bad[0]} ({C.STEP_KINDS[bad[0]]}), coefficients {bad[1]}"
        else:
            written = [s for s in range(C.STEPS) if dev[i][s] is not None]
            assert not written, f"{name} n={N_REAL}: killed pair {i} has lines written at steps {written[:8]}"


def test_line_kernels_agree(line_tables):
    """The same 68 lines: the three tables are equal mod p, coefficient by
    coefficient (tb_quad.h's steps are tb_lines.h's on more lanes; none of them
    rescales a line)."""
    w2, quad, duo = (line_tables(v)[1] for v in (0, 1, 2))
    for name, other in (("k_miller_lines_quad", quad), ("k_miller_lines_duo", duo)):
        for i in range(N_REAL):
            for s in range(C.STEPS):
                assert other[i][s] == w2[i][s], f"{name} against k_miller_lines_w2, n={N_REAL}: pair {i}, step {s}"


def test_gsettle_msg_lines(hook, real):
    """m = 70 messages: the lines at the unit point P = (1, 1); a skipped
    message's column stays unwritten."""
    skipped = {3, 63, 69}
    skip = [2 if g in skipped else 0 for g in range(N_REAL)]
    dev = C.dec_line_table(hook.msg_lines(real.Qs, skip), N_REAL)
    for g in range(N_REAL):
        if g in skipped:
            assert dev[g] == [None] * C.STEPS, f"k_gsettle_msg_lines m={N_REAL}: skipped message {g} has lines written"
        else:
            bad = C.line_mismatch(dev[g], C.ref_lines((1, 1), real.Qs[g]))
            assert bad is None, f"k_gsettle_msg_lines m={N_REAL}: message {g}, step {bad[0]}, coefficients {bad[1]}"


@pytest.mark.parametrize("variant", sorted(LINE_KERNELS), ids=[LINE_KERNELS[v] for v in sorted(LINE_KERNELS)])
def test_chain_on_real_pairs(hook, real, line_tables, variant):
    """lines -> k_miller_accs_lds (8, 4) -> the product levels -> the combine,
    as partial_run::miller and product_tree queue them: the result is the
    product of O.miller_loop over the live pairs up to Fp2; for the w2 lines
    it also pairs to e(g1, g2)^(sum a b) times the hashed pairs' pairings."""
    name = LINE_KERNELS[variant]
    per, nseg = 8, 4
    G = (N_REAL + per - 1) // per
    raw_f, _ = hook.acc(2, line_tables(variant)[0], real.flags, N_REAL, per, nseg)
    n1 = (G + 3) // 4
    lvl1 = hook.prod_seg_raw(raw_f, nseg * G, G, G, nseg, G, 4, n1, n1)
    segv = hook.prod_seg_raw(lvl1, nseg * n1, n1, n1, nseg, n1, 16, 1, 1)
    got = hook.combine_raw(segv, nseg)
    bad = C.fp2_defect(got, real.miller_product)
    assert bad is None, f"{name} -> k_miller_accs_lds ({per},{nseg}) -> products -> combine, n={N_REAL}: ratio coordinate {bad} not in Fp2"
    if variant == 0:
        assert O.final_exponentiation(got) == real.pairing, f"{name} chain: the pairing of the result"


def test_miller_wave_flags(hook, real):
    """Six pairs, one killed by each flag: a killed pair gives exactly
    (1, 0, ..., 0), a live one O.miller_loop up to Fp2."""
    idx = [1, 2, 66, 5, 67, 9]
    Ps, Qs = [real.Ps[i] for i in idx], [real.Qs[i] for i in idx]
    flags = ([0, 1, 0, 0, 0, 0], [0, 0, 0, 2, 0, 0], [0, 0, 0, 0, 0, 0xFF])
    got = hook.miller_wave(Ps, Qs, flags)
    for k, v in enumerate(C.valid_of(flags)):
        if v:
            assert got[k] is not None, f"k_miller_wave n=6: pair {k} unwritten"
            bad = C.fp2_defect(got[k], O.miller_loop(Ps[k], Qs[k]))
            assert bad is None, f"k_miller_wave n=6: live pair {k}, ratio coordinate {bad} not in Fp2"
        else:
            assert got[k] == O.F12_ONE, f"k_miller_wave n=6: killed pair {k} is not exactly one"


# ---- accumulators on synthetic tables ------------------------------------------------------------
N_SYN = 133


@pytest.fixture(scope="module")
def synth():
    """133 columns of random lines; raw(n): the table of the first n columns."""
    tabs = C.random_lines(N_SYN, seed=17)

    @functools.lru_cache(maxsize=None)
    def raw(n):
        return C.enc_line_table(tabs[:n])

    return tabs, raw


def _check_acc(hook, synth, variant, n, per, nseg, special=True):
    tabs, raw = synth
    name = f"{ACC_KERNELS[variant]} n={n} per={per} nseg={nseg}"
    groups = C.groups_strided(n, per) if variant == 2 else C.groups_contiguous(n, per)
    flags = C.kill_flags(n, groups if special else [], seed=100 * per + nseg)
    if not special:  # the case is about the mask's last bit: group 0 is full and its last pair is live
        assert len(groups[0]) == per
        for f in flags:
            f[groups[0][-1]] = 0
    valid = C.valid_of(flags)
    want = C.ref_acc(tabs[:n], valid, groups, nseg)
    _, got = hook.acc(variant, raw(n), flags, n, per, nseg)
    for j in range(nseg):
        for g, own in enumerate(groups):
            live = [i for i in own if valid[i]]
            assert got[j][g] is not None, f"{name}: segment {j}, group {g} (pairs {own}) unwritten"
            assert got[j][g] == want[j][g], f"{name}: segment {j} (steps {C.seg_bounds(j, nseg)}), group {g}, pairs {own}, live {live}"


def test_miller_acc1(hook, synth):
    _check_acc(hook, synth, 0, N_SYN, 1, 1)


def test_miller_acc2(hook, synth):
    """n = 133: the last thread owns one pair."""
    _check_acc(hook, synth, 1, N_SYN, 2, 1)


@pytest.mark.parametrize("per,nseg", [(2, 1), (4, 1), (2, 3), (8, 4), (16, 5), (32, 16)])
def test_miller_accs_lds(hook, synth, per, nseg):
    """Every f_out slot of every segment; with seg_stride = G a padded lane's
    write would land in the next segment's slots or, for the last, in the
    guard.  The first groups have 0, 1, 2, 3 and all of their pairs valid: the
    fresh, sparse, two-line and two-line-then-sparse paths."""
    _check_acc(hook, synth, 2, N_SYN, per, nseg)


@pytest.mark.parametrize("per,nseg,n", [(16, 5, 127), (32, 16, 95)])
def test_miller_accs_lds_last_mask_bit(hook, synth, per, nseg, n):
    """At n = 133 a group of 16 or 32 never owns its last pair ((per - 1) G >= n:
    G = 9 and 5), so those shapes above cannot see a lost bit per - 1 of the
    mask.  Here (per - 1) G < n -- n = 127: G = 8, n = 95: G = 3 -- with about a
    quarter of the pairs killed and no group emptied."""
    assert (per - 1) * ((n + per - 1) // per) < n
    _check_acc(hook, synth, 2, n, per, nseg, special=False)


def test_miller_accs_lds_settle_shape(hook, synth):
    """settle_sets' launch: 2 x 37 pairs, per 2, 16 segments -- thread g owns
    pairs g and g + 37."""
    assert C.groups_strided(74, 2)[36] == [36, 73]
    _check_acc(hook, synth, 2, 74, 2, 16)


def test_miller_accs_gsettle(hook, synth):
    """Positions [30, 100) of 100 over 5 messages, 16 segments: line 1 from the
    message table with b scaled by set_P.x and c by set_P.y, line 2 from the
    chunk's signature table unless sskip; a position dead by set_code,
    sig_code, msg_skip, a set index >= n or a message index >= m is exactly
    one; positions outside the chunk stay unwritten."""
    tabs, _ = synth
    n, m, lo, cn, nseg = 100, 5, 30, 70, 16
    rng = random.Random(23)
    mtabs, stabs = tabs[:m], tabs[m : m + cn]
    grp_sets = list(range(n))
    rng.shuffle(grp_sets)
    msg_of_pos = sorted(rng.randrange(m) for _ in range(n))
    set_P = [(C.random_fp(rng), C.random_fp(rng)) for _ in range(n)]
    set_code, sig_code, msg_skip, sskip = [0] * n, [0] * n, [0] * m, [0] * cn
    grp_sets[lo + 9], grp_sets[lo + 64] = n + 3, 0xFFFFFFFF  # i >= n
    msg_of_pos[lo + 11] = m  # g >= m
    set_code[grp_sets[lo + 2]], sig_code[grp_sets[lo + 63]], sig_code[grp_sets[lo + 69]] = 1, 2, 1
    msg_skip[msg_of_pos[lo + 40]] = 1
    for k in (0, 5, 31, 64, 68):
        sskip[k] = 1
    got = hook.accs_gsettle(C.enc_line_table(mtabs), m, msg_of_pos, grp_sets, set_P, set_code, sig_code, msg_skip, C.enc_line_table(stabs),
                            sskip, lo, cn, n, nseg)
    kinds = set()
    for t in range(n):
        name = f"k_miller_accs_gsettle n={n} m={m} lo={lo} cn={cn} nseg={nseg}: position {t}"
        if not lo <= t < lo + cn:
            assert all(got[j * n + t] is None for j in range(nseg)), name + " outside the chunk was written"
            continue
        i, g, k = grp_sets[t], msg_of_pos[t], t - lo
        dead = i >= n or g >= m or set_code[i] or sig_code[i] or msg_skip[g]
        kinds.add("dead" if dead else "one line" if sskip[k] else "two lines")
        cols = []
        if not dead:
            px, py = set_P[i]
            cols.append([(a, O.f2_mul_fp(b, px), O.f2_mul_fp(c, py)) for a, b, c in mtabs[g]])
            if not sskip[k]:
                cols.append(stabs[k])
        for j in range(nseg):
            want = O.F12_ONE if dead else O.f12_conj(C.ref_segment(cols, *C.seg_bounds(j, nseg)))
            assert got[j * n + t] == want, f"{name} (set {i}, message {g}), segment {j}"
    assert kinds == {"dead", "one line", "two lines"}


def test_gsettle_prep(hook):
    """A CSR with groups of 1, 2 and 70 sets in two chunks: msg_of_pos,
    negr = -[r] g1, the copied signature and sskip (1 when the set is dead by
    its codes, its message is skipped, its index is >= n, or its signature is
    not used), position by position; what a chunk does not own stays unwritten."""
    n, m = 73, 3
    grp_off = [0, 1, 3, 73]
    rng = random.Random(29)
    grp_sets = list(range(n))
    rng.shuffle(grp_sets)
    for pos, s in ((5, 0), (45, 1)):  # the sets of the edge randomizers: one in each chunk, in the group of 70
        at = grp_sets.index(s)
        grp_sets[at], grp_sets[pos] = grp_sets[pos], grp_sets[at]
    grp_sets[50] = n  # a set index out of range: dead
    checked = set()
    rands = [1, (1 << 64) - 1] + [rng.getrandbits(64) or 1 for _ in range(n - 2)]
    sig_aff = bytes(rng.randrange(256) for _ in range(192 * n))  # copied, never computed with
    sig_use, set_code, sig_code, msg_skip = [1] * n, [0] * n, [0] * n, [0, 1, 0]
    for i in (4, 40):
        sig_use[i] = 0
    set_code[7], sig_code[8], sig_code[60] = 1, 3, 1
    msg = [g for g in range(m) for _ in range(grp_off[g], grp_off[g + 1])]
    for lo, cn in ((0, 40), (40, 33)):
        name = f"k_gsettle_prep n={n} m={m} lo={lo} cn={cn}"
        mop, negr, sigq, sskip = hook.gsettle_prep(grp_off, grp_sets, m, n, lo, cn, rands, sig_aff, sig_use, set_code, sig_code, msg_skip)
        for t in range(n):
            word = int.from_bytes(mop[4 * t : 4 * t + 4], "little")
            assert word == (msg[t] if lo <= t < lo + cn else 0xEEEEEEEE), f"{name}: msg_of_pos[{t}]"
        for k in range(cn):
            t, i = lo + k, grp_sets[lo + k]
            use = i < n and not set_code[i] and not sig_code[i] and not msg_skip[msg[t]] and sig_use[i] != 0
            assert sskip[k] == (0 if use else 1), f"{name}: sskip of position {t} (set {i})"
            if use:
                checked.add(rands[i])
                assert C.dec_g1(negr[96 * k : 96 * k + 96]) == C.g1_neg(C.g1_mul(rands[i])), f"{name}: negr of position {t}, r = {hex(rands[i])}"
                assert sigq[192 * k : 192 * k + 192] == sig_aff[192 * i : 192 * i + 192], f"{name}: sigq of position {t} (set {i})"
            else:
                assert negr[96 * k : 96 * k + 96] == bytes([EE]) * 96, f"{name}: negr of unused position {t} written"
                assert sigq[192 * k : 192 * k + 192] == bytes([EE]) * 192, f"{name}: sigq of unused position {t} written"
    assert {1, (1 << 64) - 1} <= checked  # the edge randomizers were compared


# ---- products and the combine -------------------------------------------------------------------
@pytest.fixture(scope="module")
def values():
    return C.random_f12_values(16 * 37, seed=31)


def _chunk_products(vals, chunk, blocks):
    return [C.ref_product(vals[b * chunk : (b + 1) * chunk]) if b * chunk < len(vals) else None for b in range(blocks)]


@pytest.mark.parametrize("n,chunk,grid", [(37, 16, 3), (37, 1, 37), (1, 16, 1), (17, 16, 4)])
def test_fp12_prod_wave(hook, values, n, chunk, grid):
    """Every chunk's product; (17, 16) on a grid of 4: blocks 2 and 3 write nothing."""
    got = hook.prod(values, n, chunk, grid)
    want = _chunk_products(values[:n], chunk, grid)
    for b in range(grid):
        assert got[b] == want[b], f"k_fp12_prod_wave n={n} chunk={chunk} grid={grid}: block {b}" + ("" if want[b] else " must write nothing")


@pytest.mark.parametrize("nseg,n,n_last,in_stride,chunk,out_stride", [(3, 20, 23, 32, 8, 5), (16, 37, 37, 37, 16, 3)],
                         ids=["last segment longer", "settle shape"])
def test_fp12_prod_wave_seg(hook, values, nseg, n, n_last, in_stride, chunk, out_stride):
    in_count = (nseg - 1) * in_stride + n_last
    grid_x = (max(n, n_last) + chunk - 1) // chunk
    raw = hook.prod_seg_raw(b"".join(C.enc_f12(v) for v in values[:in_count]), in_count, n, n_last, nseg, in_stride, chunk, grid_x, out_stride)
    count = (nseg - 1) * out_stride + grid_x
    got = C.dec_f12s(raw, count)
    want = [None] * count
    for y in range(nseg):
        seg = values[y * in_stride : y * in_stride + (n_last if y + 1 == nseg else n)]
        for b, v in enumerate(_chunk_products(seg, chunk, grid_x)):
            want[y * out_stride + b] = v
    for k in range(count):
        assert got[k] == want[k], (f"k_fp12_prod_wave_seg nseg={nseg} n={n} n_last={n_last} in_stride={in_stride} chunk={chunk} "
                                   f"out_stride={out_stride}: segment {k // out_stride}, block {k % out_stride}")


@pytest.mark.parametrize("nseg", NSEGS)
def test_fp12_seg_combine(hook, values, nseg):
    """R = v_0, then R = R^(2^d_j) v_j: exact against the Horner reference."""
    vals = values[40 : 40 + nseg]
    got = hook.combine_raw(b"".join(C.enc_f12(v) for v in vals), nseg)
    assert got == C.ref_combine(vals), f"k_fp12_seg_combine_coop nseg={nseg}"


# ---- the settle shape on real sets ---------------------------------------------------------------
@pytest.mark.parametrize("forged", [(0, 15, 16, 36), (36,)], ids=["forged 0 15 16 36", "forged 36"])
def test_settle_shape_on_real_sets(hook, forged):
    """settle_sets and settle_tail on 37 sets as 74 pairs: k_settle_mask and
    the lines, k_miller_accs_lds (74, 2, 16), the two k_fp12_prod_wave_seg
    levels, k_group_test_coop on V (all 37), A (all 3) and B.  A verdict is 1
    exactly when its group holds no forged set.  Set 20 is forged too but has
    set_code != 0: masked, it contributes 1 to its groups -- its own value
    tests 1, and with forged = (36,) its groups A[1] passes."""
    n, nseg, coded = 37, 16, 20
    Ps, Qs = C.settle_sets(n, forged=set(forged) | {coded})
    set_code = [0] * (2 * n)  # the code rows cover the 2n pairs; the signature pairs' entries are 0
    set_code[coded] = 5
    skip = hook.settle_mask(set_code[:n], n, [0] * (2 * n))
    assert skip == [1 if i == n + coded else 0 for i in range(2 * n)], "k_settle_mask n=37"
    flags = (skip, set_code, [0] * (2 * n))
    lines = hook.lines(0, Ps, Qs, flags)
    rawV, V = hook.acc(2, lines, flags, 2 * n, 2, nseg)
    assert all(V[j][coded] == O.F12_ONE for j in range(nseg)), "the masked set's value is exactly one in every segment"
    nA, nB = 3, 1
    rawA = hook.prod_seg_raw(rawV, nseg * n, n, n, nseg, n, 16, nA, nA)
    rawB = hook.prod_seg_raw(rawA, nseg * nA, nA, nA, nseg, nA, 16, nB, nB)
    clean = lambda members: 0 if any(g in forged for g in members) else 1  # noqa: E731
    got = hook.group_test(rawV, n, nseg, list(range(n)))
    assert got == [clean([g]) for g in range(n)], ("k_group_test_coop on V, stride 37, nseg 16", got)
    got = hook.group_test(rawA, nA, nseg, [0, 1, 2])
    assert got == [clean(range(16 * a, min(n, 16 * a + 16))) for a in range(nA)], ("k_group_test_coop on A, stride 3, nseg 16", got)
    got = hook.group_test(rawB, nB, nseg, [0])
    assert got == [clean(range(n))], ("k_group_test_coop on B, stride 1, nseg 16", got)
