"""The KZG transcript pin search: every (blob, commitment,
proof) triple the reference's JSON fixtures hold was run through the KZG
oracle (tools/kzg_fixture_scan.py, result committed as
tests/golden/kzg/fixture_scan.json).  None verifies -- the fixtures' blobs are
random bytes whose 32-byte words are not canonical field elements, so
verify_blob_kzg_proof returns C_KZG_BADARGS -- and KZG transcript parity stays
"unpinned".  The fixtures' blobs are stored beside the result, and the scan of
every triple is re-run on them and must match the committed result."""

import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "tests", "golden", "kzg", "fixture_scan.json")
BLOBS = os.path.join(ROOT, "tests", "golden", "kzg", "fixture_blobs")


def test_committed_scan_has_no_verifying_triple():
    d = json.load(open(SCAN))
    assert d["summary"]["triples"] == 20 and d["summary"]["verifying"] == 0
    for e in d["files"]:
        for t in e["triples"]:
            assert t["blob_canonical"] is False and t["verify_blob_kzg_proof"] == "error code 1"  # C_KZG_BADARGS


def test_scan_reproduces_from_stored_blobs():
    """Every triple of the committed scan, run again through the scan's own
    per-triple code (tools/kzg_fixture_scan.py triple_report) on the blob
    stored under tests/golden/kzg/fixture_blobs/<sha256>.bin (the 10 distinct
    blobs of the 20 triples), must give the committed entry.  Recomputed from
    the blob: `blob_sha256`, `blob_canonical` and `verify_blob_kzg_proof`;
    `commitment` and `proof` are read from the committed entry and echoed.
    Not exercised here: the scan's walk over a reference tree and its JSON /
    hex extraction (`triples`, `hexb`, `main`), which need that tree."""
    spec = importlib.util.spec_from_file_location("kzg_fixture_scan", os.path.join(ROOT, "tools", "kzg_fixture_scan.py"))
    scan = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scan)
    want = json.load(open(SCAN))
    setup = scan.load_setup()
    try:
        got = []
        for e in want["files"]:
            for t in e["triples"]:
                blob = open(os.path.join(BLOBS, t["blob_sha256"] + ".bin"), "rb").read()
                got.append(scan.triple_report(setup, t["index"], blob, bytes.fromhex(t["commitment"]), bytes.fromhex(t["proof"])))
    finally:
        setup.close()
    assert got == [t for e in want["files"] for t in e["triples"]]
    assert {"triples": len(got), "verifying": sum(1 for t in got if t["verify_blob_kzg_proof"] is True)} == want["summary"]
