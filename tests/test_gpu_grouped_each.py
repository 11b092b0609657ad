"""Per-set verdicts of a failed grouped batch, settled from the grouped pass
(tbls_batch_verify_each_grouped; tb_lib.hip settle_grouped, k_gsettle.hip).

The checker is C.verify_each (oracle/c_oracle.py) on the ungrouped sets: a
set's verdict does not depend on the other sets, so the oracle runs once over
each fixture and again only over the sets a case replaces.  Every call uses
force=True unless a case says otherwise, every test asserts from
native.group_plan which pass the shape takes, and from the tbls_stats deltas
that one pipeline and at most one settle ran, with no per-set pass.  The
return code, *ok and the verdicts are compared with tbls_batch_verify_each's
on the same arguments."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = max(1, min(16, os.cpu_count() or 1))
SIZES = [1, 2, 31, 32, 33, 64, 65, 600]


@pytest.fixture(scope="module")
def S():
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import native, synth

    native.lib()
    return synth


def _oracle_each(pk, ms, sg):
    """pk[i]: the set's key bytes (48 B per key; empty: no keys)"""
    return C.verify_each([[p[48 * k : 48 * k + 48] for k in range(len(p) // 48)] for p in pk], ms, sg, threads=THREADS)


def _run(S, pk, ms, sg, r, force=True, grouped=True, pipelines=1, n_gpus=0):
    """Both entries on the same arguments: (ok, verdicts) of the grouped one,
    after asserting the plan, the counters and the equality with
    tbls_batch_verify_each (return code, *ok, verdicts)."""
    from teku_amd import native

    L = native.lib()
    n = len(pk)
    nk = [len(p) // 48 for p in pk]
    m = len({ms[i] for i in range(n) if nk[i]})
    plan = native.group_plan(sum(1 for k in nk if k), m)[0]
    assert (plan >= (1 if force else 2)) is grouped, (n, m, plan)
    arr = S.SetArray(b"".join(pk), nk, b"".join(ms), [len(x) for x in ms], b"".join(sg))
    rr = (ctypes.c_uint64 * max(1, n))(*r)
    ok_g, ok_p = ctypes.c_int(-1), ctypes.c_int(-1)
    each_g, each_p = (ctypes.c_int * max(1, n))(), (ctypes.c_int * max(1, n))()
    before = native.stats()
    rc_g = L.tbls_batch_verify_each_grouped(arr.ptr, n, rr, n_gpus, native.GROUP_FORCE if force else 0, ctypes.byref(ok_g), each_g, None)
    after = native.stats()
    rc_p = L.tbls_batch_verify_each(arr.ptr, n, rr, n_gpus, ctypes.byref(ok_p), each_p, None)
    assert rc_g == rc_p == native.SUCCESS
    assert (ok_g.value, list(each_g[:n])) == (ok_p.value, list(each_p[:n]))
    d = {k: after[k] - before[k] for k in after}
    live = 1 if any(nk) else 0
    assert d["partials"] == pipelines * live and d["each_passes"] == 0 and d["settled"] == (0 if ok_g.value or not live else 1), d
    if n == sum(1 for k in nk if k):
        assert ok_g.value == int(all(each_g[:n]) and n > 0)
    return ok_g.value == 1, [v == 1 for v in each_g[:n]]


@pytest.fixture(scope="module")
def edges(S):
    """tests/test_gpu_grouped.py's edge batch, built here: 828 sets in 8 groups
    of SIZES sets, interleaved, over messages of 0 / 1 / 32 / 300 bytes.  828
    is no multiple of 64 or 16: 52 level-A groups and 4 level-B groups of the
    settle, and the message groups straddle wave and workgroup boundaries.
    pos: the CSR, position -> set (groups by first appearance, sets ascending)."""
    x32, y300 = S.bench_message(7, 0), S.bench_message(7, 1) * 9 + b"tail-of-300!"
    roots = [b"", b"\x07", x32, y300, x32 + b"z", b"\x08", S.bench_message(7, 2), y300[:299] + b"?"]
    left, grp = list(SIZES), []
    while any(left):
        for g in range(8):
            if left[g]:
                left[g] -= 1
                grp.append(g)
    n = len(grp)
    assert n == 828 and grp[:8] == list(range(8))
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    ms = [roots[g] for g in grp]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    members = [[i for i in range(n) if grp[i] == g] for g in range(8)]
    pos = [i for x in members for i in x]
    base = _oracle_each(pk, ms, sg)
    assert base == [True] * n
    return dict(n=n, grp=grp, sks=sks, pk=pk, ms=ms, sg=sg, r=S.random_multipliers(n), roots=roots, members=members, pos=pos)


def _check(S, e, pk, sg, changed):
    """the edge batch with the sets `changed` replaced: verdicts == the oracle's"""
    exp = [True] * e["n"]
    sub = sorted(changed)
    for i, v in zip(sub, _oracle_each([pk[i] for i in sub], [e["ms"][i] for i in sub], [sg[i] for i in sub])):
        exp[i] = v
    ok, got = _run(S, pk, e["ms"], sg, e["r"])
    assert got == exp, [i for i in range(e["n"]) if got[i] != exp[i]]
    assert ok is all(exp)
    return exp


def test_all_valid_runs_no_settle(S, edges):
    e = edges
    ok, got = _run(S, e["pk"], e["ms"], e["sg"], e["r"])  # asserts settled == 0 for a passing batch
    assert ok is True and got == [True] * e["n"]


PLACES = {
    "the 1-set group": lambda e: e["members"][0][0],
    "first of the 600 group": lambda e: e["members"][7][0],
    "last of the 600 group": lambda e: e["members"][7][-1],
    "position 15": lambda e: e["pos"][15],
    "position 16": lambda e: e["pos"][16],
    "position 255": lambda e: e["pos"][255],
    "position 256": lambda e: e["pos"][256],
}


@pytest.mark.parametrize("place", sorted(PLACES))
def test_one_bad_set(S, edges, place):
    e = edges
    j = PLACES[place](e)
    g = e["grp"][j]
    kinds = {
        "sig on another message": (None, S.sign_blob([e["sks"][j]], [e["roots"][(g + 1) % 8]])),
        "zero sig": (None, bytes(96)),
        "non-G2 sig": (None, S.NOT_IN_G2),
        "infinity sig": (None, S.INFINITY_G2),
        "infinity key": (S.INFINITY_G1, None),
        "BAD_PK": (S.BAD_PK, None),
    }
    for name, (key, sig) in kinds.items():
        pk, sg = list(e["pk"]), list(e["sg"])
        if key is not None:
            pk[j] = key
        if sig is not None:
            sg[j] = sig
        exp = _check(S, e, pk, sg, [j])
        assert exp[j] is False, (name, place)


def test_a_whole_group_invalid(S, edges):
    e = edges
    a, b = e["members"][1]
    sg = list(e["sg"])
    sg[a], sg[b] = bytes(96), S.sign_blob([e["sks"][b]], [e["roots"][0]])
    exp = _check(S, e, e["pk"], sg, [a, b])
    assert not exp[a] and not exp[b]


def test_two_signatures_of_one_group_swapped(S, edges):
    e = edges
    a, b = e["members"][5][3], e["members"][5][40]
    sg = list(e["sg"])
    sg[a], sg[b] = sg[b], sg[a]
    exp = _check(S, e, e["pk"], sg, [a, b])
    assert [i for i, v in enumerate(exp) if not v] == sorted([a, b])


def test_three_of_four_level_b_groups_fail(S, edges):
    """level-B groups are positions [0, 256), [256, 512), [512, 768), [768, 828)"""
    e = edges
    bad = [e["pos"][t] for t in (3, 100, 255, 300, 511, 800, 827)]
    pk, sg = list(e["pk"]), list(e["sg"])
    for k, i in enumerate(bad):
        if k % 3 == 0:
            sg[i] = e["sg"][(i + 1) % e["n"]]
        elif k % 3 == 1:
            sg[i] = S.NOT_IN_G2
        else:
            pk[i] = S.BAD_PK
    exp = _check(S, e, pk, sg, bad)
    assert [i for i, v in enumerate(exp) if not v] == sorted(bad)


def test_exceptional_sums_with_a_failure(S):
    """A, negA (the key of r - sk) and B under one message with equal
    randomizers: the group's key sum passes through infinity; one bad set"""
    m, m2 = S.bench_message(9, 0), S.bench_message(9, 1)
    sk = [S.interop_sk(i) for i in range(4)]
    neg0 = S.R_ORDER - sk[0]
    keys = S.pubkeys(sk + [neg0])
    sig = lambda k, msg: S.sign_blob([k], [msg])  # noqa: E731
    sets = [(keys[0], m, sig(sk[0], m)), (keys[4], m, sig(neg0, m)), (keys[1], m, sig(sk[1], m)), (keys[2], m2, sig(sk[2], m2)),
            (keys[3], m, sig(sk[3], m2))]
    r = 0x9E3779B97F4A7C15
    pk, ms, sg = [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets]
    assert _oracle_each(pk, ms, sg) == [True, True, True, True, False]
    ok, got = _run(S, pk, ms, sg, [r, r, r, 5, 99])
    assert ok is False and got == [True, True, True, True, False]


def test_degenerate_shapes(S, edges):
    from teku_amd import native

    e = edges
    # n = 0: ok 0, the return code compared in _run
    assert _run(S, [], [], [], [], grouped=False) == (False, [])
    # one set
    assert _run(S, e["pk"][:1], e["ms"][:1], e["sg"][:1], e["r"][:1], grouped=False) == (True, [True])
    # m == n = 128, one bad set: not grouped; the wave Miller loops leave no lines, so the ungrouped settle re-stages (2 pipelines)
    pks, msgs, sigs = S.single_signer(0, 128, seed=12)
    assert native.group_plan(128, 128)[0] == 0
    pk = [pks[48 * i : 48 * i + 48] for i in range(128)]
    ms = [msgs[32 * i : 32 * i + 32] for i in range(128)]
    sg = [sigs[96 * i : 96 * i + 96] for i in range(128)]
    sg[77] = sg[78]
    exp = _oracle_each(pk, ms, sg)
    assert [i for i, v in enumerate(exp) if not v] == [77]
    assert _run(S, pk, ms, sg, S.random_multipliers(128), grouped=False, pipelines=2) == (False, exp)
    # one message, 256 sets, the last signature bad
    m = S.bench_message(11, 0)
    blob = S.sign_blob(e["sks"][:256], [m] * 256)
    sg = [blob[96 * i : 96 * i + 96] for i in range(256)]
    sg[255] = sg[254]
    assert _run(S, e["pk"][:256], [m] * 256, sg, e["r"][:256]) == (False, [True] * 255 + [False])


def test_a_set_without_keys(S, edges):
    """300 sets over 7 messages, set 123 with n_pks == 0: verdict 0 and *ok 0,
    the set left out of the batch; the others as the oracle says (one is bad)"""
    e = edges
    n = 300
    roots = [S.bench_message(19, g) for g in range(7)]
    ms = [roots[i % 7] for i in range(n)]
    blob = S.sign_blob(e["sks"][:n], ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    pk = list(e["pk"][:n])
    pk[123] = b""
    sg[200] = sg[207]
    exp = [True] * n
    exp[123], exp[200] = False, _oracle_each([pk[200]], [ms[200]], [sg[200]])[0]
    assert exp[200] is False
    assert _run(S, pk, ms, sg, e["r"][:n]) == (False, exp)
    # and with every other set valid: still *ok 0, no settle (the batch itself passes)
    sg[200] = blob[96 * 200 : 96 * 201]
    exp[200] = True
    from teku_amd import native

    before = native.stats()
    arr = S.SetArray(b"".join(pk), [len(p) // 48 for p in pk], b"".join(ms), [32] * n, b"".join(sg))
    assert arr.batch_verify_each_grouped(e["r"][:n], force=True) == (False, exp)
    after = native.stats()
    assert after["partials"] - before["partials"] == 1 and after["settled"] == before["settled"]


def test_split_miller_pass(S):
    """4,096 sets over 2,048 messages: 2,112 pairs, past TB_MILLER_WAVE_MAX, so
    the grouped pass ran its line kernel; the last set bad"""
    from teku_amd import native

    n, m = 4096, 2048
    assert native.group_plan(n, m)[1] == 2112
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    roots = [S.bench_message(13, g) for g in range(m)]
    ms = [roots[i % m] for i in range(n)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    sg[n - 1] = sg[n - 2]
    assert _oracle_each(pk[-1:], ms[-1:], sg[-1:]) == [False]
    assert _run(S, pk, ms, sg, S.random_multipliers(n)) == (False, [True] * (n - 1) + [False])


def test_without_force(S):
    """2,304 sets over 40 messages group by the thresholds alone"""
    from teku_amd import native

    n, m = 2304, 40
    assert native.group_plan(n, m)[0] == 2
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    roots = [S.bench_message(21, g) for g in range(m)]
    ms = [roots[(7 * i) % m] for i in range(n)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    bad = [0, 1000, 2303]
    sg[0], sg[1000], sg[2303] = sg[1], bytes(96), sg[2302]
    assert _oracle_each([pk[i] for i in bad], [ms[i] for i in bad], [sg[i] for i in bad]) == [False] * 3
    assert _run(S, pk, ms, sg, S.random_multipliers(n), force=False) == (False, [i not in bad for i in range(n)])


@pytest.mark.parametrize("n,m", [(16640, 65), (33024, 129)])
def test_the_other_signature_line_kernels(S, n, m):
    """The signature pairs' lines come from the line kernel a batch of that
    many pairs takes (tb_plan.h line_group): lane quads up to 16,384 pairs (every
    other test), lane pairs up to 32,768, one lane above.  One shard (n_gpus =
    1), keys cyclic over 4,096; bad sets first, in the middle and last."""
    K = 4096
    sks = [S.interop_sk(i) for i in range(K)]
    keys = S.pubkeys(sks)
    roots = [S.bench_message(23, g) for g in range(m)]
    ms = [roots[i % m] for i in range(n)]
    blob = S.sign_blob([sks[i % K] for i in range(n)], ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    pk = [keys[i % K] for i in range(n)]
    bad = [0, n // 2, n - 1]
    sg[0], sg[n // 2], sg[n - 1] = sg[1], S.INFINITY_G2, sg[n - 2]
    assert _oracle_each([pk[i] for i in bad], [ms[i] for i in bad], [sg[i] for i in bad]) == [False] * 3
    ok, got = _run(S, pk, ms, sg, S.random_multipliers(n), n_gpus=1)
    assert ok is False and [i for i in range(n) if not got[i]] == bad


def test_key_table_loaded(S):
    """512 byte-keyed sets over 8 messages, every key in a 1,024-key table: one
    set names a key whose table status is invalid, one has a bad signature"""
    from teku_amd import native

    L = native.lib()
    n, m, K = 512, 8, 1024
    sks = [S.interop_sk(i) for i in range(K)]
    table = S.pubkeys(sks)
    table[700] = S.BAD_PK
    native.check(L.tbls_pk_table_load(b"".join(table), K, None), "pk_table_load")
    try:
        idx = [(2 * i + 1) % K for i in range(n)]
        idx[77] = 700
        roots = [S.bench_message(15, g) for g in range(m)]
        ms = [roots[(3 * i) % m] for i in range(n)]
        blob = S.sign_blob([sks[k] for k in idx], ms)
        sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
        sg[400] = sg[401]
        pk = [table[k] for k in idx]
        exp = [i not in (77, 400) for i in range(n)]
        assert _oracle_each([pk[77], pk[400]], [ms[77], ms[400]], [sg[77], sg[400]]) == [False, False]
        assert _run(S, pk, ms, sg, S.random_multipliers(n)) == (False, exp)
    finally:
        native.check(L.tbls_pk_table_clear(), "pk_table_clear")


def test_service_with_group_settle(S):
    """2,048 one-set tasks over 16 messages, 3 of them bad: one device pass"""
    from teku_amd import native
    from teku_amd.service import AggregatingSignatureVerificationService, SignatureTask

    n, m = 2048, 16
    assert native.group_plan(n, m)[0] >= 1
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    roots = [S.bench_message(17, g) for g in range(m)]
    ms = [roots[(5 * i) % m] for i in range(n)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    sg[0], sg[1000], sg[2047] = sg[1], bytes(96), sg[2046]
    bad = [0, 1000, 2047]
    assert _oracle_each([pk[i] for i in bad], [ms[i] for i in bad], [sg[i] for i in bad]) == [False] * 3
    exp = [i not in bad for i in range(n)]
    svc = AggregatingSignatureVerificationService(num_threads=1, max_batch_size=n, group_messages=True, group_force=True, group_settle=True)
    tasks = [SignatureTask([(pk[i], 1, ms[i], sg[i])]) for i in range(n)]
    before = native.stats()
    svc.batch_verify_signatures(tasks)
    after = native.stats()
    assert [t.result.result(timeout=60) for t in tasks] == exp
    assert after["partials"] - before["partials"] == 1 and after["settled"] - before["settled"] == 1 and after["each_passes"] == before["each_passes"]
    mt = svc.metrics()
    assert mt["grouped_batches_total"] == 1 and mt["device_passes_total"] == 1 and svc.last_batch_timing["settled"] is True
    good = [SignatureTask([(pk[i], 1, ms[i], sg[i])]) for i in range(1, 1000)]
    svc.batch_verify_signatures(good)
    assert all(t.result.result(timeout=60) for t in good) and svc.metrics()["device_passes_total"] == 2
    assert svc.last_batch_timing["settled"] is False


def test_chunks_and_two_shards():
    """tools/grouped_each_probe.py in a fresh process: 1,024 sets over 8
    messages in two shards of 512 on one GPU, each settled in two chunks of 256"""
    env = dict(os.environ, TBLS_SHARD_MIN="256", TBLS_GSETTLE_CHUNK="256")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grouped_each_probe.py")], capture_output=True, text=True, timeout=300, env=env,
                       cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(lines[-1])
    print(r)
    assert r["devices"] == 2 and r["shard_min"] == 256 and r["group_plan"][0] >= 1
    both, one = r["cases"]
    assert both["bad"] == [255, 256, 700] and one["bad"] == [700]
    for c in (both, one):
        assert c["n_devices"] == 2 and c["partials"] == 2 and c["each_passes"] == 0, c
        assert c["ok"] is False and c["mismatch"] == [] and c["rc"] == c["rc_plain"] == 0, c
        assert c["failed"] == c["bad"], c
    assert both["settled"] == 2 and one["settled"] == 1
    assert p.returncode == 0, p.stderr[-2000:]
