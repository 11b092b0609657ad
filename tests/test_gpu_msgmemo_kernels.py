"""k_memo_fill and k_memo_learn (teku_amd/csrc/k_msgmemo.hip) byte for byte:
the product library's own kernels, launched through the test hook
(tests/native/k_test_memo.hip) with the library's grid on random byte arrays,
against a numpy gather.

Shapes: n = 1, 5, 64, 65 and 1,000 pairs over m_hash = 0, 1, 3 and 70 hashed
entries and 4 rows, src mixing both sources (rows only when nothing is
hashed), with set_grp (an ungrouped pass: pairs are sets, several per group)
and without (a grouped pass: pair i is group i).  Q and skip carry 3 entries
of padding behind the n pairs: those bytes, and the rows that learn does not
name, must stay as they were."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW, NONE, ROWS, PAD = 0x80000000, 0xFFFFFFFF, 4, 3


@pytest.fixture(scope="module")
def hook():
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import native
    from tests.opcodec import load_test_lib

    native.lib()
    L = load_test_lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.tbls_test_memo.restype = ctypes.c_int
    L.tbls_test_memo.argtypes = [ctypes.c_char_p, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, u32, u32, vp, vp]
    so = native.LIB_PATH.encode()

    def run(src, set_grp, n, qh, skiph, learn, rows, row_skip, q, skip):
        ptr = lambda a: None if a is None else a.ctypes.data_as(vp)  # noqa: E731
        rc = L.tbls_test_memo(so, ptr(src), len(src), ptr(set_grp), n, ptr(qh), ptr(skiph), len(skiph), ptr(learn), ptr(rows), ptr(row_skip),
                              ROWS, PAD, ptr(q), ptr(skip))
        assert rc == 0, "hook returned %d" % rc

    return run


@pytest.mark.parametrize("with_set_grp", [True, False])
@pytest.mark.parametrize("m_hash", [0, 1, 3, 70])
@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_fill_and_learn_bytes(hook, n, m_hash, with_set_grp):
    rng = np.random.default_rng(1000 * n + 10 * m_hash + with_set_grp)
    n_groups = max(1, min(n, 37)) if with_set_grp else n
    # every source appears when there is room: rows and hashed entries in turn, then random
    pick = lambda g: (ROW | (g % ROWS)) if (m_hash == 0 or g % 2 == 0) else (g // 2) % m_hash  # noqa: E731
    src = np.array([pick(g) if g < 2 * (ROWS + m_hash) else (ROW | int(rng.integers(ROWS)) if m_hash == 0 or rng.random() < 0.5 else int(rng.integers(m_hash)))
                    for g in range(n_groups)], dtype=np.uint32)
    set_grp = np.concatenate([np.arange(n_groups), rng.integers(n_groups, size=n)])[:n].astype(np.uint32) if with_set_grp else None
    if with_set_grp:
        rng.shuffle(set_grp)
    qh = rng.integers(256, size=(m_hash, 192), dtype=np.uint8)
    skiph = rng.integers(2, size=m_hash, dtype=np.uint8)
    learn = np.full(m_hash, NONE, dtype=np.uint32)
    named = rng.permutation(ROWS)[: min(m_hash, 2)]  # at most two rows are learned, by the last hashed entries
    for k, r in enumerate(named):
        learn[m_hash - 1 - k] = r
    rows0 = rng.integers(256, size=(ROWS, 192), dtype=np.uint8)
    rskip0 = rng.integers(2, size=ROWS, dtype=np.uint8)
    q0 = rng.integers(256, size=(n + PAD, 192), dtype=np.uint8)
    skip0 = rng.integers(256, size=n + PAD, dtype=np.uint8)
    rows, rskip, q, skip = rows0.copy(), rskip0.copy(), q0.copy(), skip0.copy()
    hook(src, set_grp, n, qh, skiph, learn, rows, rskip, q, skip)
    # the gather, from the arrays as they were before the learn
    grp = set_grp if with_set_grp else np.arange(n)
    w = src[grp]
    from_row = (w & ROW) != 0
    e = (w & ~np.uint32(ROW)).astype(np.int64)
    want_q, want_skip = q0.copy(), skip0.copy()
    for i in range(n):
        want_q[i] = rows0[e[i]] if from_row[i] else qh[e[i]]
        want_skip[i] = rskip0[e[i]] if from_row[i] else skiph[e[i]]
    want_rows, want_rskip = rows0.copy(), rskip0.copy()
    for j in range(m_hash):
        if learn[j] != NONE:
            want_rows[learn[j]] = qh[j]
            want_rskip[learn[j]] = skiph[j]
    assert np.array_equal(q[:n], want_q[:n]) and np.array_equal(skip[:n], want_skip[:n])
    assert np.array_equal(q[n:], q0[n:]) and np.array_equal(skip[n:], skip0[n:]), "bytes outside Q[0..n) changed"
    assert np.array_equal(rows, want_rows) and np.array_equal(rskip, want_rskip)
    untouched = [r for r in range(ROWS) if r not in set(int(x) for x in learn if x != NONE)]
    assert all(np.array_equal(rows[r], rows0[r]) and rskip[r] == rskip0[r] for r in untouched)
