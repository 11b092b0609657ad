"""The host side of grouped batches on the CPU: the grouping of a batch's sets
by message and the grouped staging image (teku_amd/csrc/tb_group.h), and the
grouped batch plan (teku_amd/csrc/tb_plan.h).  Host builds of
tests/native/group_check.cpp and group_plan_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer, as stand-alone programs.

The expectation of the grouping and of the image is built here from the
format's statement alone, not from the code under test: two messages are the
same when length and bytes are equal; groups are numbered by first appearance
in the range; the CSR lists each group's sets rebased to the range's first
set, ascending; the image has the regions keys, key offsets, messages (the
distinct ones, in group order), message offsets (m + 1), signatures,
randomizers, DST, CSR offsets (m + 1), CSR sets (n; 1 word when n is 0), each
at a multiple of 256 bytes, empty message / DST regions taking 1 byte.  Bytes
the format leaves unwritten still hold the marker."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0xA5
SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-I", os.path.join(ROOT, "teku_amd", "csrc")]


def pat(tag, i, n):
    return bytes((tag * 61 + i * 17 + j * 7 + 3) & 0xFF for j in range(n))


def rand_of(i):
    return (0x0102030405060708 * (i + 1) + i) & (2**64 - 1)


def align(x):
    return (x + 255) // 256 * 256


def expected(msgs, lo, hi, with_rand, dlen):
    """(set_grp, offsets, total, image, m, M) of sets [lo, hi); set i has one
    48-byte key and signs msgs[i]"""
    n = hi - lo
    distinct, set_grp = [], []
    for i in range(lo, hi):
        if msgs[i] not in distinct:
            distinct.append(msgs[i])
        set_grp.append(distinct.index(msgs[i]))
    m = len(distinct)
    members = [[i for i in range(n) if set_grp[i] == g] for g in range(m)]
    grp_off = [0]
    for g in range(m):
        grp_off.append(grp_off[-1] + len(members[g]))
    grp_sets = [i for g in range(m) for i in members[g]]
    keys = b"".join(pat(1, i, 48) for i in range(lo, hi))
    koff = list(range(n + 1))
    mbytes = b"".join(distinct)
    moff = [0]
    for d in distinct:
        moff.append(moff[-1] + len(d))
    sigs = b"".join(pat(3, i, 96) for i in range(lo, hi))
    rnd = b"".join(struct.pack("<Q", rand_of(i) if with_rand else 1) for i in range(lo, hi))
    u32 = lambda v: struct.pack("<%dI" % len(v), *v)
    regions = [(keys, len(keys)), (u32(koff), 4 * (n + 1)), (mbytes, max(len(mbytes), 1)), (u32(moff), 4 * (m + 1)), (sigs, 96 * n),
               (rnd, 8 * n), (pat(4, 0, dlen), max(dlen, 1)), (u32(grp_off), 4 * (m + 1)), (u32(grp_sets), max(4 * n, 4))]
    offs, o = [], 0
    for _, size in regions:
        offs.append(o)
        o = align(o + size)
    image = bytearray([MARK]) * o
    for off, (data, _) in zip(offs, regions):
        image[off:off + len(data)] = data
    return set_grp, offs, o, bytes(image), m, len(mbytes)


# name -> (messages of all sets, lo, hi, randomizers given, DST bytes): as tests/native/group_check.cpp spells them
CASES = {
    "empty": ([], 0, 0, False, 43),
    "distinct": ([b"alpha", b"beta", b"gamma!"], 0, 3, True, 43),
    "equal_ptr": ([b"same-root"] * 4, 0, 4, False, 43),
    "equal_bytes": ([b"same-root"] * 3, 0, 3, True, 0),
    "same_ptr_lens": ([b"abcdefgh", b"abcd", b"abcdefgh", b"abcd", b""], 0, 5, True, 43),
    "zero_len": ([b"", b"x", b"", b""], 0, 4, False, 43),
    "all_zero_len": ([b"", b""], 0, 2, False, 43),
    "range_1_3": ([b"outside", b"inner", b"inner", b"outside"], 1, 3, True, 43),
}


def build_and_run(tmp, name):
    exe = str(tmp / name)
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    got = {}
    for ln in build_and_run(tmp_path_factory.mktemp("group"), "group_check").splitlines():
        got[ln.split()[1]] = dict(kv.split("=") for kv in ln.split()[2:])
    return got


def test_every_case_is_printed(images):
    assert sorted(images) == sorted(CASES)


def test_the_stated_groupings():
    """the expectation itself, by hand, for the cases the grouping turns on"""
    assert expected(*CASES["same_ptr_lens"])[0] == [0, 1, 0, 1, 2]
    assert expected(*CASES["zero_len"])[0] == [0, 1, 0, 0]
    assert expected(*CASES["range_1_3"])[0] == [0, 0]
    set_grp, offs, total, image, m, M = expected(*CASES["same_ptr_lens"])
    assert (m, M) == (3, 12) and offs == [0, 256, 512, 768, 1024, 1536, 1792, 2048, 2304] and total == 2560
    assert image[2048:2064] == struct.pack("<4I", 0, 2, 4, 5) and image[2304:2324] == struct.pack("<5I", 0, 2, 1, 3, 4)


@pytest.mark.parametrize("name", sorted(CASES))
def test_grouping_and_image_match_the_format(images, name):
    msgs, lo, hi, with_rand, dlen = CASES[name]
    set_grp, offs, total, image, m, M = expected(msgs, lo, hi, with_rand, dlen)
    f = images[name]
    assert (int(f["n"]), int(f["m"]), int(f["K"]), int(f["M"])) == (hi - lo, m, hi - lo, M)
    assert ([] if f["set_grp"] == "-" else [int(x) for x in f["set_grp"].split(",")]) == set_grp
    assert [int(x) for x in f["off"].split(",")] == offs
    assert int(f["total"]) == total
    got = bytes.fromhex(f["image"])
    assert len(got) == total
    if got != image:
        bad = [i for i in range(total) if got[i] != image[i]]
        pytest.fail("%d bytes differ, first at %d: got %02x want %02x" % (len(bad), bad[0], got[bad[0]], image[bad[0]]))


def test_grouped_plan(tmp_path_factory):
    """tests/native/group_plan_check.cpp checks the plan itself and prints one
    line per failed check; `ok <count>` when none failed"""
    out = build_and_run(tmp_path_factory.mktemp("gplan"), "group_plan_check")
    last = out.strip().splitlines()[-1]
    assert last.startswith("ok "), out[-4000:]
    assert int(last.split()[1]) > 1000
