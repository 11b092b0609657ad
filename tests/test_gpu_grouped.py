"""Grouped batches on the GPU: sets that sign the same message share one
hash_to_G2 and one Miller loop (tb_group.h, tb_plan.h grouped plans,
k_group_pk_sum_coop, tbls_batch_verify_grouped and its siblings).

The checker is C.batch_verify (oracle/c_oracle.py) on the UNGROUPED sets with
the same randomizers: the grouped product equals the ungrouped one in GT, so
every verdict must equal the oracle's.  Every grouped call uses force=True and
every test asserts from tbls_group_plan that the shape is a grouped one, so
the path under test is the new one."""
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
SIZES = [1, 2, 31, 32, 33, 64, 65, 600]  # a copy; one row each; one short of / exactly / one past the 32 rows; two walks; past them; many walks


@pytest.fixture(scope="module")
def S():
    import torch  # noqa: F401  (share torch's HIP runtime)

    from teku_amd import native, synth

    native.lib()
    return synth


def _grouped(S, pk, ms, sg, r):
    from teku_amd import native

    n, m = len(pk), len(set(ms))
    grouped, pairs = native.group_plan(n, m)
    assert grouped >= 1 and pairs == m + 64, (n, m, grouped, pairs)  # the grouped pass runs under force
    return S.SetArray(b"".join(pk), [1] * n, b"".join(ms), [len(x) for x in ms], b"".join(sg)).batch_verify_grouped(r, force=True)


def _oracle(pk, ms, sg, r):
    return C.batch_verify(pk, ms, sg, r, threads=THREADS)


@pytest.fixture(scope="module")
def edges(S):
    """828 sets in 8 groups of SIZES sets, interleaved (the groups take turns
    until each is full), over messages of 0, 1, 32 and 300 bytes, two pairs of
    them sharing a prefix; keys are interop keys 0..827, one per set"""
    x32, y300 = S.bench_message(7, 0), S.bench_message(7, 1) * 9 + b"tail-of-300!"
    roots = [b"", b"\x07", x32, y300, x32 + b"z", b"\x08", S.bench_message(7, 2), y300[:299] + b"?"]
    assert [len(x) for x in roots] == [0, 1, 32, 300, 33, 1, 32, 300] and len(set(roots)) == 8
    left, grp = list(SIZES), []
    while any(left):
        for g in range(8):
            if left[g]:
                left[g] -= 1
                grp.append(g)
    n = len(grp)
    assert n == 828 and grp[:8] == list(range(8)) and grp[-1] == 7
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    ms = [roots[g] for g in grp]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    return dict(n=n, grp=grp, sks=sks, pk=pk, ms=ms, sg=sg, r=S.random_multipliers(n), roots=roots)


def test_group_sizes_at_the_kernels_edges(S, edges):
    e = edges
    assert _grouped(S, e["pk"], e["ms"], e["sg"], e["r"]) is _oracle(e["pk"], e["ms"], e["sg"], e["r"]) is True


@pytest.mark.parametrize("group", [4, 7])  # the 33-set and the 600-set group
def test_tampered_set_inside_a_group(S, edges, group):
    e = edges
    members = [i for i, g in enumerate(e["grp"]) if g == group]
    j = members[len(members) // 2]
    cases = {}
    s = list(e["sg"])
    s[j] = S.sign_blob([e["sks"][j]], [e["roots"][(group + 1) % 8]])
    cases["sig on another message"] = (e["pk"], s)
    for name, bad in [("zero sig", bytes(96)), ("infinity sig", S.INFINITY_G2), ("non-G2 sig", S.NOT_IN_G2)]:
        s = list(e["sg"])
        s[j] = bad
        cases[name] = (e["pk"], s)
    for name, bad in [("infinity key", S.INFINITY_G1), ("0x9378a6 key", S.BAD_PK)]:
        p = list(e["pk"])
        p[j] = bad
        cases[name] = (p, e["sg"])
    for name, (p, s) in cases.items():
        got, exp = _grouped(S, p, e["ms"], s, e["r"]), _oracle(p, e["ms"], s, e["r"])
        assert got is exp is False, (name, group, j)


def test_exceptional_sums(S):
    """P == +-Q inside a group is ordinary input here; randomizers chosen by
    the test.  A key's negation is the key of r - sk."""
    m, m2 = S.bench_message(9, 0), S.bench_message(9, 1)
    sk = [S.interop_sk(i) for i in range(4)]
    neg0 = S.R_ORDER - sk[0]
    keys = S.pubkeys(sk + [neg0])
    sig = lambda k, msg: S.sign_blob([k], [msg])  # noqa: E731
    A = (keys[0], m, sig(sk[0], m))
    negA = (keys[4], m, sig(neg0, m))
    B = (keys[1], m, sig(sk[1], m))
    other = (keys[2], m2, sig(sk[2], m2))  # a second message: the shapes stay grouped ones with a finite pair as well
    bad = (S.BAD_PK, m, sig(sk[3], m))      # an invalid set: its key fails the checks, its point is left out of the sum
    r = 0x9E3779B97F4A7C15
    cases = {
        "P == Q": ([A, A, other], [r, r, 5], True),
        "P == -Q: the sum is infinity": ([A, negA, other], [r, r, 5], True),
        "P == -Q alone": ([A, negA], [r, r], None),  # one message: m = 1, the pair is skipped
        "three, the first two cancel": ([A, negA, B, other], [r, r, 77, 5], True),
        "the same with an invalid set": ([A, negA, B, bad, other], [r, r, 77, 99, 5], False),
    }
    for name, (sets, rr, want) in cases.items():
        pk, ms, sg = [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets]
        got, exp = _grouped(S, pk, ms, sg, rr), _oracle(pk, ms, sg, rr)
        assert got is exp, name
        if want is not None:
            assert got is want, name
    assert _grouped(S, [A[0], negA[0]], [m, m], [A[2], negA[2]], [r, r]) is True


def test_degenerate_groupings(S, edges):
    from teku_amd import native

    e = edges
    # one message, 256 sets
    m = S.bench_message(11, 0)
    sks = e["sks"][:256]
    blob = S.sign_blob(sks, [m] * 256)
    sg = [blob[96 * i : 96 * i + 96] for i in range(256)]
    r = e["r"][:256]
    assert _grouped(S, e["pk"][:256], [m] * 256, sg, r) is _oracle(e["pk"][:256], [m] * 256, sg, r) is True
    s = list(sg)
    s[255] = sg[254]
    assert _grouped(S, e["pk"][:256], [m] * 256, s, r) is _oracle(e["pk"][:256], [m] * 256, s, r) is False
    # one set: nothing repeats, the entry runs the existing pass
    assert native.group_plan(1, 1)[0] == 0
    one = S.SetArray(e["pk"][0], [1], m, [32], sg[0])
    assert one.batch_verify_grouped([r[0]], force=True) is one.batch_verify([r[0]]) is C.verify_each([[e["pk"][0]]], [m], [sg[0]])[0] is True
    # m = n = 128: every message distinct -> not grouped, the verdict is the existing pass's
    pks, msgs, sigs = S.single_signer(0, 128, seed=12)
    assert native.group_plan(128, 128) == (0, 256)
    arr = S.SetArray.single(pks, msgs, sigs)
    r128 = S.random_multipliers(128)
    pk = [pks[48 * i : 48 * i + 48] for i in range(128)]
    ms = [msgs[32 * i : 32 * i + 32] for i in range(128)]
    sg = [sigs[96 * i : 96 * i + 96] for i in range(128)]
    assert arr.batch_verify_grouped(r128, force=True) is arr.batch_verify(r128) is _oracle(pk, ms, sg, r128) is True
    # n = 0: false, as tbls_batch_verify (BLS.java:240-241)
    empty = S.SetArray(b"", [], b"", [], b"")
    assert empty.batch_verify_grouped([], force=True) is empty.batch_verify([]) is False
    # a set with no keys: TBLS_BAD_ARGUMENT from both entries
    nokeys = S.SetArray(e["pk"][0] + e["pk"][1], [1, 0, 1], m * 3, [32, 32, 32], sg[0] + sg[1] + sg[1])
    for call in (lambda: nokeys.batch_verify_grouped([1, 2, 3], force=True), lambda: nokeys.batch_verify([1, 2, 3])):
        with pytest.raises(ValueError):
            call()


def test_split_miller_path(S):
    """4,096 sets over 2,048 messages: 2,112 pairs, past TB_MILLER_WAVE_MAX, so
    the line kernel, the accumulator and the product levels run"""
    from teku_amd import native

    n, m = 4096, 2048
    assert native.group_plan(n, m)[1] == 2112
    sks = [S.interop_sk(i) for i in range(n)]
    pk = S.pubkeys(sks)
    roots = [S.bench_message(13, g) for g in range(m)]
    ms = [roots[i % m] for i in range(n)]
    blob = S.sign_blob(sks, ms)
    sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
    r = S.random_multipliers(n)
    assert _grouped(S, pk, ms, sg, r) is _oracle(pk, ms, sg, r) is True
    s = list(sg)
    s[n - 1] = sg[n - 2]  # the last group's second set
    assert _grouped(S, pk, ms, s, r) is _oracle(pk, ms, s, r) is False


def _idx_sets(native, idx_lists, ms, sg):
    n = len(ms)
    arr = (native.TblsSetIdx * n)()
    keep = []
    for i in range(n):
        ib = (ctypes.c_uint32 * len(idx_lists[i]))(*idx_lists[i])
        mb, sb = ctypes.create_string_buffer(ms[i], len(ms[i])), ctypes.create_string_buffer(sg[i], 96)
        keep += [ib, mb, sb]
        arr[i].key_idx = ctypes.cast(ib, ctypes.c_void_p)
        arr[i].n_pks = len(idx_lists[i])
        arr[i].msg = ctypes.cast(mb, ctypes.c_void_p)
        arr[i].msg_len = len(ms[i])
        arr[i].sig = ctypes.cast(sb, ctypes.c_void_p)
    return arr, keep


def test_table_keys(S, edges):
    """tbls_batch_verify_idx_grouped over a 1,024-key table: 512 sets, 8
    messages, one invalid table key named by one set"""
    from teku_amd import native

    L = native.lib()
    n, m, K = 512, 8, 1024
    sks = [S.interop_sk(i) for i in range(K)]
    table = S.pubkeys(sks)
    BAD = 700
    table[BAD] = S.BAD_PK
    native.check(L.tbls_pk_table_load(b"".join(table), K, None), "pk_table_load")
    try:
        assert native.group_plan(n, m)[0] >= 1
        idx = [(2 * i + 1) % K for i in range(n)]  # odd table indices: not the first n keys
        roots = [S.bench_message(15, g) for g in range(m)]
        ms = [roots[(3 * i) % m] for i in range(n)]
        blob = S.sign_blob([sks[k] for k in idx], ms)
        sg = [blob[96 * i : 96 * i + 96] for i in range(n)]
        r = S.random_multipliers(n)
        rr = (ctypes.c_uint64 * n)(*r)

        def both(idx_list):
            arr, keep = _idx_sets(native, [[k] for k in idx_list], ms, sg)
            ok_g, ok_p = ctypes.c_int(-1), ctypes.c_int(-1)
            rc_g = L.tbls_batch_verify_idx_grouped(arr, n, rr, 0, native.GROUP_FORCE, ctypes.byref(ok_g), None)
            rc_p = L.tbls_batch_verify_idx(arr, n, rr, 0, ctypes.byref(ok_p), None)
            assert rc_g == rc_p
            return rc_g, ok_g.value, ok_p.value

        assert both(idx) == (native.SUCCESS, 1, 1)
        assert _oracle([table[k] for k in idx], ms, sg, r) is True
        named = list(idx)
        named[77] = BAD  # one set names the invalid key
        assert both(named) == (native.SUCCESS, 0, 0)
        assert _oracle([table[k] for k in named], ms, sg, r) is False
        past = list(idx)
        past[5] = K  # an index past the table
        assert both(past)[0] == native.BAD_ARGUMENT
    finally:
        native.check(L.tbls_pk_table_clear(), "pk_table_clear")


def test_two_shards_every_group_straddles_the_cut():
    env = dict(os.environ, TBLS_SHARD_MIN="256")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grouped_shards_probe.py")], capture_output=True, text=True, timeout=300, env=env,
                       cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(lines[-1])
    print(r)
    assert r["devices"] == 2 and r["shard_min"] == 256
    assert r["group_plan"][0] >= 1 and r["group_plan"][1] == 4 + 64  # each shard: 256 sets, 4 messages
    valid, bad = r["cases"]
    for c in (valid, bad):
        assert c["n_devices"] == 2 and c["partials"] == 2, c
        assert c["got"] is c["plain"] is c["oracle"], c
    assert valid["got"] is True and bad["got"] is False
    assert p.returncode == 0, p.stderr[-2000:]


def test_device_entry(S, edges):
    """tbls_dev_batch_partial_grouped + tbls_dev_final_verify on the edge-size
    batch: the host entry's verdict, and the invalid-set count of
    tbls_dev_batch_partial's record on the same sets"""
    import torch

    from teku_amd import native

    L = native.lib()
    e = edges
    n = e["n"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    u8 = lambda b: torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev)  # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    offs = lambda lens: [sum(lens[:k]) for k in range(len(lens) + 1)]  # noqa: E731
    rand = torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in e["r"]], dtype=torch.int64, device=dev)
    members = [[i for i in range(n) if e["grp"][i] == g] for g in range(8)]
    grp_off, grp_sets = i32(offs([len(x) for x in members])), i32([i for x in members for i in x])
    assert native.group_plan(n, 8)[0] >= 1

    def records(sg, pk):
        keys, sigs, pk_off = u8(b"".join(pk)), u8(b"".join(sg)), i32(list(range(n + 1)))
        msgs_u, off_u = u8(b"".join(e["ms"])), i32(offs([len(x) for x in e["ms"]]))
        msgs_g, off_g = u8(b"".join(e["roots"])), i32(offs([len(x) for x in e["roots"]]))
        plain = native.TblsDevBatch(keys.data_ptr(), pk_off.data_ptr(), n, msgs_u.data_ptr(), off_u.data_ptr(), sigs.data_ptr(), rand.data_ptr(), n)
        grouped = native.TblsDevBatch(keys.data_ptr(), pk_off.data_ptr(), n, msgs_g.data_ptr(), off_g.data_ptr(), sigs.data_ptr(), rand.data_ptr(), n)
        out = torch.zeros(2, native.PARTIAL_BYTES, dtype=torch.uint8, device=dev)
        native.check(L.tbls_dev_batch_partial_grouped(0, ctypes.byref(grouped), None, 8, grp_off.data_ptr(), grp_sets.data_ptr(), stream,
                                                      out[0].data_ptr()), "partial_grouped")
        native.check(L.tbls_dev_batch_partial(0, ctypes.byref(plain), stream, out[1].data_ptr()), "partial")
        oks = []
        for k in range(2):
            ok = ctypes.c_int(-1)
            native.check(L.tbls_dev_final_verify(0, out[k].data_ptr(), 1, stream, ctypes.byref(ok)), "final")
            oks.append(ok.value)
        torch.cuda.synchronize()
        host = out.cpu().numpy().tobytes()
        n_bad = [int.from_bytes(host[k * native.PARTIAL_BYTES + 576 : k * native.PARTIAL_BYTES + 580], "little") for k in range(2)]
        return oks, n_bad

    oks, n_bad = records(e["sg"], e["pk"])
    assert oks == [1, 1] and n_bad == [0, 0]
    assert _grouped(S, e["pk"], e["ms"], e["sg"], e["r"]) is True
    sg, pk = list(e["sg"]), list(e["pk"])
    sg[100], sg[500], pk[300] = bytes(96), S.NOT_IN_G2, S.BAD_PK  # two undecodable signatures and an invalid key: three invalid sets
    oks, n_bad = records(sg, pk)
    assert oks == [0, 0] and n_bad[0] == n_bad[1] == 3
    assert _grouped(S, pk, e["ms"], sg, e["r"]) is False
    # every message distinct, or none: not a grouped launch
    d = native.TblsDevBatch(0, 0, n, 0, 0, 0, 0, n)
    for bad_m in (0, n, n + 1):
        assert L.tbls_dev_batch_partial_grouped(0, ctypes.byref(d), None, bad_m, grp_off.data_ptr(), grp_sets.data_ptr(), stream, 0) == native.BAD_ARGUMENT


def test_service_with_group_messages(S):
    """2,048 one-set tasks over 16 messages, 3 of them bad: per-task verdicts
    equal C.verify_each; the failed grouped batch went on to the per-set pass"""
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
    exp = C.verify_each([[p] for p in pk], ms, sg, threads=THREADS)
    assert [i for i, v in enumerate(exp) if not v] == [0, 1000, 2047]
    svc = AggregatingSignatureVerificationService(num_threads=1, max_batch_size=n, group_messages=True, group_force=True)
    tasks = [SignatureTask([(pk[i], 1, ms[i], sg[i])]) for i in range(n)]
    svc.batch_verify_signatures(tasks)
    assert [t.result.result(timeout=60) for t in tasks] == exp
    mt = svc.metrics()
    assert mt["grouped_batches_total"] == 1 and mt["grouped_sets_per_message"] == n / m and mt["device_passes_total"] == 2
    # and a valid batch stays on the grouped entry
    good = [SignatureTask([(pk[i], 1, ms[i], sg[i])]) for i in range(1, 1000)]
    svc.batch_verify_signatures(good)
    assert all(t.result.result(timeout=60) for t in good) and svc.metrics()["device_passes_total"] == 3
