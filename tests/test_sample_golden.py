"""CPU: the Python restatement of gzfastq_sample (sample_ref.py) against what the reference recorded in
tests/golden/sample/ (make_golden_sample.py) -- it is the checker of the GPU tests' random inputs, so it is pinned
to the reference first."""
import gzip
import hashlib
import json
import os

import pytest

import sample_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "sample", "manifest.json")))


def read_input(rel):
    raw = open(os.path.join(GOLDEN, rel), "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def check_outputs(case, got):
    """got: {file name: decompressed bytes, or None for a 0-byte file} against the recorded outputs."""
    assert sorted(got) == [o["name"] for o in case["outputs"]]
    for o in case["outputs"]:
        text = got[o["name"]]
        assert (text is None) == o["empty_file"], o["name"]
        text = text or b""
        assert len(text) == o["size"], o["name"]
        assert hashlib.sha256(text).hexdigest() == o["sha256"], o["name"]
        if o["data"]:
            assert text == open(os.path.join(GOLDEN, "sample", o["data"]), "rb").read()


def test_manifest_covers_the_ground():
    ids = {c["id"] for c in CASES}
    assert len(ids) == len(CASES) >= 70
    assert any(c["in2"] for c in CASES) and any("-f" in c["args"] for c in CASES)
    assert any(o["empty_file"] for c in CASES for o in c["outputs"])
    assert all(c["rc"] == 0 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_matches_the_reference(case):
    got, err = sample_ref.simulate(case["args"], os.path.basename(case["in1"]), read_input(case["in1"]),
                                   os.path.basename(case["in2"]) if case["in2"] else None, read_input(case["in2"]) if case["in2"] else None)
    check_outputs(case, got)
    assert err == case["stderr"]


def test_x31_takes_bytes_as_signed_chars():
    assert sample_ref.x31(b"") == 0 and sample_ref.x31(b"@") == 64
    assert sample_ref.x31(b"\xc3\xa9") == ((0xc3 - 256) * 31 + (0xa9 - 256)) & 0xFFFFFFFF


def test_threshold_is_the_float_comparison():
    for frac in (1e-8, 0.25, 0.3, 0.5785, 0.999, 1.0, 2.5):
        t = sample_ref.threshold(frac)
        for k in {0, 1, max(t - 1, 0), min(t, (1 << 24) - 1), (1 << 24) - 1}:
            assert (k / (1 << 24) < frac) == (k < t)
