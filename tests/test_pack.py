"""The staging image of a host batch (teku_amd/csrc/tb_pack.h: the offset /
stride contract between the host's packing and the kernels) on the CPU: host
build of tests/native/pack_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program.

The program packs each case into a block pre-filled with a marker byte and
prints the offsets and the block.  The expectation here is built from the
format's statement alone, not from the code under test: regions in the order
keys, key offsets, messages, message offsets, signatures, randomizers, DST;
each region starts at a multiple of 256 bytes; empty message and DST regions
take 1 byte; n + 1 offsets (little-endian u32), rebased to the range's first
set; randomizers as little-endian u64, 1 when none is given; a bit row
zero-padded to its stride in 4-byte words.  Bytes the format leaves unwritten
still hold the marker."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0xA5


def pat(tag, i, n):
    """the program's input bytes: field `tag` of set i, n bytes"""
    return bytes((tag * 61 + i * 17 + j * 7 + 3) & 0xFF for j in range(n))


def rand_of(i):
    return (0x0102030405060708 * (i + 1) + i) & (2**64 - 1)


def align(x):
    return (x + 255) // 256 * 256


def expected(key_len, msg_len, lo, hi, dlen, key_unit, with_rand, row_bytes=None):
    """(offsets, total, image) of sets [lo, hi): set i has key_len[i] bytes of
    keys (key_unit bytes per offset unit; bit rows: row_bytes each, padded to
    key_len[i]) and msg_len[i] message bytes."""
    n = hi - lo
    keys, koff, msgs, moff, sigs, rnd = b"", [0], b"", [0], b"", b""
    for i in range(lo, hi):
        k = pat(1, i, key_len[i]) if row_bytes is None else pat(1, i, row_bytes) + bytes(key_len[i] - row_bytes)
        keys += k
        koff.append(len(keys) // key_unit)
        msgs += pat(2, i, msg_len[i])
        moff.append(len(msgs))
        sigs += pat(3, i, 96)
        rnd += struct.pack("<Q", rand_of(i) if with_rand else 1)
    regions = [(keys, len(keys)), (struct.pack("<%dI" % (n + 1), *koff), 4 * (n + 1)), (msgs, max(len(msgs), 1)),
               (struct.pack("<%dI" % (n + 1), *moff), 4 * (n + 1)), (sigs, 96 * n), (rnd, 8 * n), (pat(4, 0, dlen), max(dlen, 1))]
    offs, o = [], 0
    for _, size in regions:
        offs.append(o)
        o = align(o + size)
    image = bytearray([MARK]) * o
    for off, (data, _) in zip(offs, regions):
        image[off:off + len(data)] = data
    return offs, o, bytes(image)


# name -> (expected image, n, K, M)
CASES = {
    "empty": (expected([], [], 0, 0, 43, 48, False), 0, 0, 0),
    "one": (expected([48], [0], 0, 1, 0, 48, False), 1, 1, 0),
    "bytes_1_3": (expected([48, 96, 144], [0, 1, 300], 1, 3, 43, 48, True), 2, 5, 301),
    "idx_1_3": (expected([4, 8, 12], [0, 1, 300], 1, 3, 43, 4, True), 2, 5, 301),
    "bits_13": (expected([4, 4], [32, 5], 0, 2, 43, 4, False, row_bytes=2), 2, 2, 37),
    "bits_512": (expected([64, 64], [32, 5], 0, 2, 43, 4, False, row_bytes=64), 2, 32, 37),
}


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack") / "pack_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "teku_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "pack_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = {}
    for ln in out.stdout.splitlines():
        f = dict(kv.split("=") for kv in ln.split()[2:])
        got[ln.split()[1]] = f
    return got


def test_every_case_is_printed(images):
    assert sorted(images) == sorted(CASES)


def test_sub_range_offsets_are_the_stated_ones():
    offs, total, _ = CASES["bytes_1_3"][0]
    assert offs == [0, 256, 512, 1024, 1280, 1536, 1792] and total == 2048


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_matches_the_format(images, name):
    (offs, total, image), n, K, M = CASES[name]
    f = images[name]
    assert (int(f["n"]), int(f["K"]), int(f["M"])) == (n, K, M)
    assert [int(x) for x in f["off"].split(",")] == offs
    assert int(f["total"]) == total
    got = bytes.fromhex(f["image"])
    assert len(got) == total
    if got != image:
        bad = [i for i in range(total) if got[i] != image[i]]
        pytest.fail("%d bytes differ, first at %d: got %02x want %02x" % (len(bad), bad[0], got[bad[0]], image[bad[0]]))
