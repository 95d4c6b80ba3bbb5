"""CPU: the Python restatement of gzfastq_uniq (uniq_ref.py: framing, representatives, the closed form of the
hash-table walk) equals every output and stderr line recorded from the compiled reference (tests/golden/uniq/)."""
import atexit
import gzip
import hashlib
import json
import os
import shutil
import tempfile
import zlib

import pytest

import uniq_inputs
import uniq_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "uniq", "manifest.json")))
CASES = MANIFEST["cases"]
_made = []


def input_path(rel):
    """A case's input file: a file of tests/golden/fastq/, or one of tests/uniq_inputs.py -- those are made once per
    process in a temporary directory and held to the digests the recorder stored."""
    if not rel.startswith("uniq/inputs/"):
        return os.path.join(GOLDEN, rel)
    if not _made:
        _made.append(tempfile.mkdtemp(prefix="uniq_inputs_"))
        atexit.register(shutil.rmtree, _made[0], ignore_errors=True)
        uniq_inputs.materialize(_made[0], MANIFEST["inputs"])
    return os.path.join(_made[0], rel[len("uniq/inputs/"):])


def read_input(rel):
    raw = open(input_path(rel), "rb").read()
    return gzip.decompress(raw) if rel.endswith(".gz") else raw


def check_outputs(case, got, prefix="o"):
    """got: {file name: bytes}.  Every recorded file equals it (a file the reference left half written: is a prefix of it)."""
    recorded = {o["name"]: o for o in case["outputs"]}
    if case["expect"] == "same":
        assert sorted(got) == sorted(recorded)
    for name, o in recorded.items():
        text = got[name]
        if o["partial"]:
            want = o["text"].encode("latin-1")
            assert text[:len(want)] == want, name
            continue
        assert len(text) == o["size"], name
        assert hashlib.sha256(text).hexdigest() == o["sha256"], name
        if o["text"] is not None:
            assert text == o["text"].encode("latin-1"), name


def expected_files(case):
    """What the tool has to write for a case the reference answers: from the restatement (the recorded files are held
    against the same bytes by test_restatement_equals_the_reference)."""
    out, err, r = uniq_ref.simulate(read_input(case["in1"]), read_input(case["in2"]) if case["in2"] else None)
    return {"o" + k: v for k, v in out.items()}, err, r


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_equals_the_reference(case):
    if case["expect"] == "refuse":
        if not case["out"]:
            return   # (no -o: the reference dies on its second output file whatever the input)
        with pytest.raises((uniq_ref.NoAnswer, zlib.error, gzip.BadGzipFile, EOFError)):
            expected_files(case)
        return
    got, err, r = expected_files(case)
    check_outputs(case, got)
    if case["expect"] == "same":
        assert err == case["stderr"]
    else:
        assert err.startswith(case["stderr"]) and case["stderr"]


def test_the_goldens_cover_what_they_claim():
    by_id = {c["id"]: c for c in CASES}
    assert len(CASES) >= 60
    # both sides of dict.c's extra doubling, single-end and paired
    for u in (4, 8, 16, 32, 64, 128, 1024):
        assert "hash size: %d\n" % u in by_id["u%d_plain" % u]["stderr"] and "hash size: %d\n" % (2 * u) in by_id["u%d_behind" % u]["stderr"]
    for u in (4, 8, 16, 64):
        assert "hash size: %d\n" % u in by_id["pu%d_plain" % u]["stderr"] and "hash size: %d\n" % (2 * u) in by_id["pu%d_behind" % u]["stderr"]
    assert {c["id"] for c in CASES if c["expect"] == "refuse"} >= {"trunc_fq", "longname_fq", "badcrc_fq_gz", "badcrc_mid_fq_gz", "badisize_fq_gz", "shortq", "no_dash_o"}
    assert by_id["stale_fq"]["expect"] == "diverge"
    assert "error at 31: " in by_id["pe_badmid"]["stderr"] and "error at 37: " in by_id["pe_mate_short"]["stderr"]
    assert "error at" not in by_id["pe_mate_long"]["stderr"] and "error at 11: @n11\n" in by_id["pe_nospace_unequal"]["stderr"]


def test_restatement_units():
    assert uniq_ref.djb2(b"") == 5381 and uniq_ref.djb2(b"a") == 5381 * 33 + 97
    assert [uniq_ref.epoch(j) for j in (0, 3, 4, 7, 8, 15, 16)] == [0, 0, 1, 1, 2, 2, 3]
    assert uniq_ref.frame(b"@a\nAC\n+\nII\n@tail") == [(b"@a", b"AC", b"II")]       # a lone line without '\n' is no record
    assert uniq_ref.frame(b"@a\nAC\n+\nII") == [(b"@a", b"AC", b"I")]                 # the last line loses a real byte
    assert uniq_ref.sum_q(b"AC", b"I") == 73
    for bad in (b"@a\nAC\n+\nII\n@b\n", b"@a\nAC\n", b"@a\n" + b"A" * 1023 + b"\n+\nI\n"):
        with pytest.raises(uniq_ref.NoAnswer):
            uniq_ref.frame(bad)
    with pytest.raises(uniq_ref.NoAnswer):
        uniq_ref.collapse(b"@a\nACGT\n+\nII\n")
