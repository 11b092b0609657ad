"""The per-key comb rows on the GPU (teku_amd/csrc/tb_pkcomb.h,
k_pkindex.hip k_pk_learn_comb / k_pk_comb_build / k_pk_lookup_ref, k_w2_pk.hip
k_set_pk_comb_w2; tbls_pk_comb_stats).

Kernel level (tests/native/k_test_pkcomb.hip, tests/pkcomb_cases.py
kernel_batch): 130 sets -- two full 64-lane workgroups and a partial one.  The
build kernels run on hand-made rows, then k_set_pk_comb_w2 with references that
mix ready, not-ready and table-sourced rows lane by lane, k_set_pk_w2 on the
same sets, and k_set_pk_comb_w2 by index.  Every P is compared in canonical
form with oracle/bls12_381.py's scalar multiple (tests/pkcomb_cases.py
kernel_reference), codes and n_bad too; there is no tolerance.

Library level (child processes: the settings are read once per process, and
TBLS_W2_MIN=64 / TBLS_COOP=0 bring 192 sets to the two-wave key kernel, the
only place the product reads a comb row): tbls_dev_batch_partial + the final
exponentiation on 192 sets over 64 distinct keys, cold and then served by the
comb (the counter says so), the same Fp12 from both records; a corrupted
signature through tbls_batch_verify_each warm and cold; again after
tbls_pk_cache_clear; by index and by bytes after tbls_pk_table_load; with
TBLS_PK_COMB_KEYS below the key count; and with TBLS_PK_COMB=0.
"""

import ctypes
import json
import os
import subprocess
import sys

import pytest

from tests import pkcomb_cases as PC
from tests import stage_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READY, TABLE, ROW = 0x80000000, 0x40000000, 0x3FFFFFFF


# ---- kernel level ------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_case():
    batch, modes, key_idx = PC.kernel_batch()
    return batch, modes, key_idx, PC.kernel_reference(batch)


@pytest.fixture(scope="module")
def hook():
    from teku_amd import native
    from tests.opcodec import load_test_lib

    L = load_test_lib()
    vp, cp, sz, u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32
    L.tbls_test_pkcomb.restype = ctypes.c_int
    L.tbls_test_pkcomb.argtypes = [cp, cp, sz, vp, vp, sz, cp, u32, vp] + [vp] * 12
    so = native.LIB_PATH.encode()

    def run(batch, modes, key_idx, cap):
        n, K = len(batch.rands), batch.n_keys
        u32s = lambda v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
        outs = [(ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n), ctypes.c_uint32(0xEEEEEEEE)) for _ in range(3)]
        ref_lookup, ref_used, stat = (ctypes.c_uint32 * K)(), (ctypes.c_uint32 * K)(), (ctypes.c_uint64 * 4)()
        args = []
        for p, c, b in outs:
            args += [p, c, ctypes.byref(b)]
        rc = L.tbls_test_pkcomb(so, batch.blob, K, u32s(batch.pk_off), (ctypes.c_uint64 * n)(*batch.rands), n, bytes(modes), cap,
                                u32s(key_idx), *args, ref_lookup, ref_used, stat)
        if rc:  # a failed HIP call: nothing more may run on that device
            pytest.exit(f"tests/native/k_test_pkcomb.hip: HIP call failed ({rc}); no further GPU work", returncode=3)
        sets = [[(S.dec_g1(p.raw[96 * i : 96 * i + 96]), c.raw[i]) for i in range(n)] for p, c, _ in outs]
        return sets, [b.value for _, _, b in outs], list(ref_lookup), list(ref_used), list(stat)

    return run


def _assert_sets(name, batch, got, n_bad, want):
    for i, ((p, code), (wp, wcode)) in enumerate(zip(got, want)):
        assert code == wcode, (name, "set", i, batch.tags[i], "r", hex(batch.rands[i]), "set_code")
        assert p == wp, (name, "set", i, batch.tags[i], "r", hex(batch.rands[i]), "P")
    assert n_bad == sum(1 for _, c in want if c), name


@pytest.mark.parametrize("cap", [131, 40], ids=["every row", "cap 40"])
def test_comb_kernels(hook, kernel_case, cap):
    batch, modes, key_idx, want = kernel_case
    (comb, w2, by_idx), n_bad, ref_lookup, ref_used, stat = hook(batch, modes, key_idx, cap)
    _assert_sets("k_set_pk_comb_w2", batch, comb, n_bad[0], want)
    _assert_sets("k_set_pk_w2", batch, w2, n_bad[1], want)
    _assert_sets("k_set_pk_comb_w2 by index", batch, by_idx, n_bad[2], want)
    assert [c for _, c in comb] == [c for _, c in w2] and n_bad[0] == n_bad[1] == n_bad[2] == 2  # the key outside G1, r == 0
    # the lookup's references: a valid key's cache row when it lies below the cap, nothing for the invalid key
    valid = [j for j in range(batch.n_keys) if j != 5]
    ready = [j for j in valid if ref_lookup[j] & READY]
    assert ref_lookup[5] == 0 and all(ref_lookup[j] == 0 for j in valid if j not in ready)
    assert len(ready) == min(cap, 130) and sorted(ref_lookup[j] & ROW for j in ready) == list(range(len(ready)))
    assert all(not ref_lookup[j] & TABLE and (ref_lookup[j] & ROW) < cap for j in ready)
    assert stat[1] == len(ready) and stat[2] == 130  # rows built: the cache's below the cap, the table's for every valid key
    # the first wave mixes the three kinds lane by lane
    first = [ref_used[j] for j in range(64)]
    assert sum(1 for r in first if r & TABLE) >= 20 and sum(1 for r in first if r == 0) >= 21
    if cap == 131:
        assert sum(1 for r in first if r & READY and not r & TABLE) >= 20
    # sets served: single valid keys with r != 0 -- by reference in the first launch, every one of them by index
    single = [i for i in range(len(batch.rands)) if batch.pk_off[i + 1] - batch.pk_off[i] == 1 and i not in (5, 9)]
    by_ref = sum(1 for i in single if ref_used[batch.pk_off[i]] & READY)
    assert len(single) == 127 and stat[0] == by_ref + len(single)
    if cap == 131:
        assert by_ref == sum(1 for i in single if modes[batch.pk_off[i]] != 0)


def test_scalars_cover_the_comb():
    """The scalar list starts a walk at every entry, and holds the edges the issue names."""
    rs = PC.comb_scalars(130)
    assert {PC.first_entry(r) for r in rs} >= set(range(1, 16))
    assert all(r in rs for r in (1, 2, 1 << 15, 1 << 16, (1 << 16) + 1, 1 << 48, 1 << 63, (1 << 64) - 1))
    assert 0xBEEF >> 16 == 0 and all((0x7FFE7FFE7FFE7FFE >> (16 * t + j)) & 1 == 0 for t in range(4) for j in (0, 15))


# ---- library level -------------------------------------------------------------------
def _child(**env):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), TBLS_PK_CACHE_KEYS="1024", **PC.CHILD_ENV)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.pkcomb_cases"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _fp12(step):
    from teku_amd import dist

    f, n_bad = dist.decode_partial(bytes.fromhex(step["rec"]))
    assert n_bad == 0 and step["ok"] == 1
    return f


def _common(got):
    """What holds with and without comb rows: verdicts, and one Fp12 from every record."""
    N = PC.N_SETS
    want_each = [p != PC.BAD_SET for p in range(N)]
    f = _fp12(got["cold"])
    for name in ("warm", "cleared_cold", "cleared_warm", "by_index", "bytes_with_table"):
        assert _fp12(got[name]) == f, name
    for name in ("each_warm", "each_cold"):
        assert got[name]["ok"] is False and got[name]["each"] == want_each, name
    return f


@pytest.fixture(scope="module")
def library():
    return _child()


def test_library_served_by_the_comb(library):
    got, N, D = library, PC.N_SETS, PC.N_DISTINCT
    _common(got)
    assert got["cold"]["comb"] == [0, D, 0, 1024]  # every key decompressed and learned, its row built; nothing read
    assert got["warm"]["comb"] == [N, 0, 0, 1024]  # every set through a comb row
    served, built, tab, _ = got["each_warm"]["comb"]  # the batch pass, and the pass that settles the failed batch
    assert served >= N and served % N == 0 and (built, tab) == (0, 0)
    served, built, tab, _ = got["each_cold"]["comb"]  # cleared first: the batch pass learns, what follows is served
    assert served % N == 0 and (built, tab) == (D, 0)
    assert got["cleared_cold"]["comb"] == [0, D, 0, 1024] and got["cleared_warm"]["comb"] == [N, 0, 0, 1024]
    assert got["table_load"]["comb"] == [0, 0, D, 1024]
    assert got["by_index"]["comb"] == [N, 0, 0, 1024] and got["bytes_with_table"]["comb"] == [N, 0, 0, 1024]


def test_library_capped_and_off(library):
    """TBLS_PK_COMB_KEYS=40 < 64 keys: some keys never get a comb row and are
    multiplied as before; TBLS_PK_COMB=0: no row is built or read.  The records
    hold the same Fp12 as with every row."""
    f = _fp12(library["cold"])
    capped = _child(TBLS_PK_COMB_KEYS="40")
    assert _common(capped) == f
    _, built, _, cap = capped["cold"]["comb"]
    assert cap == 40 and 0 < built <= 40
    assert capped["warm"]["comb"] == [3 * built, 0, 0, 40]  # every key signs three sets
    assert capped["by_index"]["comb"][0] == PC.N_SETS  # the table's region is not capped
    off = _child(TBLS_PK_COMB="0")
    assert _common(off) == f
    assert all(step["comb"] == [0, 0, 0, 0] for step in off.values())
