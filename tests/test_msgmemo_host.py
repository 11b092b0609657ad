"""The hash-point memo's host index on the CPU (teku_amd/csrc/tb_msgmemo.h):
a host build of tests/native/msgmemo_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program, driven with R = 4 rows
through scripted and seeded random sequences of shards.

The expectation is a dictionary model of the stated rules
(tests/msgmemo_model.py), not taken from the code under test: messages of up to 64 bytes are cacheable;
a shard's distinct messages are taken in first-appearance order; `new` counts
the distinct cacheable messages that are not resident; if new <= free rows
they take the next free rows in order; otherwise the index is flushed (and
the flush counted), every distinct cacheable message of the shard is new, the
first min(count, R) take rows 0, 1, ... and the rest are hashed and not
learned.  m_hash lists the distinct messages that are not served from a row,
src[g] is ROW | r or the position in m_hash, learn[j] the row or NONE."""
import os
import random
import subprocess

import pytest

from tests.msgmemo_model import NONE, ROW, Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
       "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc")]

def msg(tag, n=32):
    return bytes((tag * 37 + j * 11 + 5) & 0xFF for j in range(n))


A, B, C, D, E, F, G = (msg(t) for t in range(1, 8))
EMPTY, M64, M65 = b"", msg(9, 64), msg(9, 65)  # the 65-byte message extends the 64-byte one

# (op, messages): the sequences the index must get right, with R = 4
SCRIPTED = [
    ("shard", [A, B, A, A, B]),             # repeats inside a shard: 2 new, rows 0 and 1
    ("shard", [B, A, C]),                   # hits across shards, and one new: row 2
    ("shard", [EMPTY]),                     # the empty message is cacheable: exactly as many new as free rows (1)
    ("shard", [EMPTY, A, EMPTY, C]),        # all four resident
    ("shard", [A, D]),                      # one more new message than free rows (0): flush, A and D from row 0
    ("shard", [M64, M65, M64, M65]),        # 64 bytes cacheable, 65 hashed every time and never learned
    ("shard", [M65, M64]),                  # the over-long one again: hashed again; the 64-byte one from its row
    ("gshard", [A, A, D, D, D]),            # a grouped pass counts one pair per distinct message
    ("shard", [B, C, E, F, G, B]),          # more than R new messages (with one free row): flush, 4 learned, the fifth hashed only
    ("shard", [G]),                         # the overflow was not learned: a full index and one new message flush again
    ("invalidate", None),
    ("shard", [G, B]),                      # invalidate() between shards: nothing resident, rows from 0
    ("shard", []),                          # no sets at all
]


def script_of(seq):
    out = ["rows 4"]
    for op, msgs in seq:
        out.append(op if msgs is None else " ".join([op] + [m.hex() if m else "-" for m in msgs]))
    return "\n".join(out) + "\n"


def random_sequence(seed):
    rng = random.Random(seed)
    pool = [msg(t, rng.choice([0, 1, 31, 32, 63, 64, 65, 96])) for t in range(20, 32)]
    seq = []
    for _ in range(120):
        if rng.random() < 0.08:
            seq.append(("invalidate", None))
        else:
            seq.append((rng.choice(["shard", "shard", "gshard"]), [rng.choice(pool[: rng.randint(1, len(pool))]) for _ in range(rng.randint(0, 9))]))
    return seq


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("msgmemo") / "msgmemo_check")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "native", "msgmemo_check.cpp"), "-o", path])
    return path


def run(exe, tmp_path, seq):
    script = tmp_path / "script.txt"
    script.write_text(script_of(seq))
    out = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = []
    for ln in out.stdout.splitlines():
        f = dict(kv.split("=") for kv in ln.split())
        for k in ("m_hash", "src", "learn"):
            f[k] = [] if f[k] == "-" else [int(x, 16) for x in f[k].split(",")]
        got.append({k: (v if isinstance(v, list) else int(v)) for k, v in f.items()})
    return got


def expect(seq):
    model, want = Model(4), []
    for op, msgs in seq:
        if op == "invalidate":
            model.invalidate()
        else:
            want.append(model.shard(msgs, op == "shard"))
    return want


def test_the_model_on_the_stated_cases():
    """the expectation itself, by hand, where the rules turn"""
    w = expect(SCRIPTED)
    assert w[0] == dict(m_hash=[0, 1], src=[0, 1], learn=[0, 1], flushed=0, hits=0, hashed=2, flushes=0, used=2)
    assert w[1]["src"] == [ROW | 1, ROW | 0, 0] and w[1]["learn"] == [2] and w[1]["hits"] == 2
    assert w[2]["learn"] == [3] and w[2]["flushed"] == 0 and w[2]["used"] == 4
    assert w[3]["m_hash"] == [] and w[3]["hits"] == 6
    assert w[4] == dict(m_hash=[0, 1], src=[0, 1], learn=[0, 1], flushed=1, hits=6, hashed=6, flushes=1, used=2)
    assert w[5]["learn"] == [2, NONE] and w[5]["used"] == 3
    assert w[6]["src"] == [0, ROW | 2] and w[6]["learn"] == [NONE]
    assert w[7]["hits"] == w[6]["hits"] + 2
    assert w[8]["flushed"] == 1 and w[8]["learn"] == [0, 1, 2, 3, NONE] and w[8]["used"] == 4
    assert w[9]["flushed"] == 1 and w[9]["learn"] == [0] and w[9]["flushes"] == 3
    assert w[10] == dict(m_hash=[0, 1], src=[0, 1], learn=[0, 1], flushed=0, hits=w[9]["hits"], hashed=w[9]["hashed"] + 2, flushes=3, used=2)
    assert w[11]["m_hash"] == [] and w[11]["src"] == []


def test_scripted_sequence(exe, tmp_path):
    assert run(exe, tmp_path, SCRIPTED) == expect(SCRIPTED)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sequences(exe, tmp_path, seed):
    seq = random_sequence(seed)
    got, want = run(exe, tmp_path, seq), expect(seq)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "shard %d" % k
    assert want[-1]["flushes"] > 0 and want[-1]["hits"] > 0  # the sequences do exercise both
