"""CPU: the Python restatement of gzfastq_sort (sort_ref.py: framing, the stable order by length and bytes, stderr, the
pipe that cannot be rewound) equals every output and stderr line recorded from the compiled reference (tests/golden/sort/)."""
import atexit
import gzip
import hashlib
import json
import os
import shutil
import tempfile
import zlib

import pytest

import sort_inputs
import sort_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "sort", "manifest.json")))
CASES = MANIFEST["cases"]
_made = []


def input_path(rel):
    """A case's input file: a file of tests/golden/fastq/, or one of tests/sort_inputs.py -- those are made once per process in
    a temporary directory and held to the digests the recorder stored."""
    if not rel.startswith("sort/inputs/"):
        return os.path.join(GOLDEN, rel)
    if not _made:
        _made.append(tempfile.mkdtemp(prefix="sort_inputs_"))
        atexit.register(shutil.rmtree, _made[0], ignore_errors=True)
        sort_inputs.materialize(_made[0], MANIFEST["inputs"])
    return os.path.join(_made[0], rel[len("sort/inputs/"):])


def read_input(rel):
    raw = open(input_path(rel), "rb").read()
    return gzip.decompress(raw) if rel.endswith(".gz") else raw


def reads_num(case):
    return sort_ref.parse_r(case["args"][case["args"].index("-r") + 1]) if "-r" in case["args"] else None


def check_blob(o, text, what):
    assert len(text) == o["size"], what
    assert hashlib.sha256(text).hexdigest() == o["sha256"], what
    if o["text"] is not None:
        assert text == o["text"].encode("latin-1"), what


def check_outputs(case, stdout, files):
    """stdout: bytes; files: {file name: bytes}.  Everything the reference wrote equals them."""
    assert sorted(files) == sorted(o["name"] for o in case["outputs"]), case["id"]
    check_blob(case["stdout"], stdout, "stdout")
    for o in case["outputs"]:
        check_blob(o, files[o["name"]], o["name"])


def expected(case):
    """(stdout, files, stderr, Result) of a case the reference answers, from the restatement."""
    if case["in"] is None:      # a missing input: the reference creates it empty
        data = b""
    else:
        data = read_input(case["in"])
    out, err, r = sort_ref.simulate(data, case["by_name"], reads_num(case), case["stdin"] != "pipe")
    prefix = case["args"][case["args"].index("-o") + 1] if "-o" in case["args"] else "-"
    if prefix.startswith("-"):
        return out, {}, err, r
    return b"", {prefix + ("_sort_by_name.fq" if case["by_name"] else "_sort_by_seq.fq"): out}, err, r


SAME = [c for c in CASES if c["expect"] == "same" and c["rc"] == 0]
REFUSE = [c for c in CASES if c["expect"] == "refuse"]


@pytest.mark.parametrize("case", SAME, ids=[c["id"] for c in SAME])
def test_restatement_equals_the_reference(case):
    stdout, files, err, r = expected(case)
    check_outputs(case, stdout, files)
    assert err == case["stderr"]
    assert r.rounds == (1 + len(r.tied) if r.n else 0) and r.refined == sum(r.tied)


@pytest.mark.parametrize("case", REFUSE, ids=[c["id"] for c in REFUSE])
def test_restatement_has_no_answer_where_the_reference_has_none(case):
    with pytest.raises((sort_ref.NoAnswer, zlib.error, gzip.BadGzipFile, EOFError)):
        expected(case)


def test_the_goldens_cover_what_they_claim():
    by_id = {c["id"]: c for c in CASES}
    assert len(CASES) >= 60
    assert {c["id"] for c in REFUSE} >= {"trunc_fq-s", "longname_fq-n", "badcrc_fq_gz-s", "badcrc_mid_fq_gz-n", "badisize_fq_gz-s", "cut_plus-s", "cut_seq-n",
                                          "cut_name-s", "r_smaller", "pipe_r_smaller"}
    assert all(c["rc"] == -11 for c in REFUSE)
    # a pipe without -r: counted, not rewound, nothing sorted
    assert by_id["pipe"]["outputs"][0]["size"] == 0 and "total_reads_num: 12\n" in by_id["pipe"]["stderr"]
    assert by_id["pipe_r"]["outputs"][0]["size"] == by_id["stdin_file"]["outputs"][0]["size"] > 0
    # no -o, and a prefix that begins with '-': standard output
    for cid in ("no_dash_o", "dash_o_dash", "pipe_r_stdout"):
        assert by_id[cid]["outputs"] == [] and by_id[cid]["stdout"]["size"] == 230
    # the last mode given wins, the default is by sequence
    assert by_id["n_then_s"]["outputs"][0]["name"] == by_id["no_mode"]["outputs"][0]["name"] == "o_sort_by_seq.fq"
    assert by_id["s_then_n"]["outputs"][0]["name"] == "o_sort_by_name.fq"
    assert "total_reads_num" not in by_id["r_exact"]["stderr"] and "total_reads_num: 12\n" in by_id["r_zero"]["stderr"] and "total_reads_num: 12\n" in by_id["r_text"]["stderr"]
    assert (by_id["r_negative"]["rc"], by_id["r_negative"]["stderr"]) == (1, "reads count must be a positive integer!\n")
    assert by_id["missing_file"]["outputs"][0]["size"] == 0
    assert by_id["nonl-s"]["outputs"][0]["size"] == by_id["small-s"]["outputs"][0]["size"] - 1      # the last line loses a real byte
    assert by_id["lone_line-s"]["stderr"].startswith("total_reads_num: 13\n")
    assert all(by_id[u]["expect"] == "usage" and by_id[u]["rc"] == 1 for u in ("usage_none", "usage_h", "usage_unknown"))


def test_the_inputs_hold_the_cases_the_refinement_needs():
    for name, by_name in (("ties40.fq", False), ("dup_names.fq", True), ("edges.fq", False), ("edges.fq", True), ("illumina.fq", True), ("hibytes.fq", True)):
        data = sort_inputs.own_inputs()[name]
        _, _, r = sort_ref.simulate(data, by_name)
        keys = [x[0 if by_name else 1] for x in sort_ref.records(data)]
        assert len(set(keys)) < len(keys), name      # ties in full
        if name == "ties40.fq":
            assert len(set(keys)) == 40 and r.refined < r.n      # (duplicates leave the refinement after one look)
        if name in ("edges.fq", "illumina.fq"):
            assert r.rounds >= 4, (name, r.tied)
    lens = {len(x[1]) for x in sort_ref.records(sort_inputs.own_inputs()["edges.fq"])}
    assert lens >= set(sort_inputs.EDGE_LENGTHS)
    assert sort_ref.simulate(sort_inputs.own_inputs()["edges.fq"], False)[2].rounds == 128      # 1022 bytes: the last round there is


def test_restatement_units():
    assert sort_ref.parse_r("20x") == 20 and sort_ref.parse_r("many") == 0 and sort_ref.parse_r("012") == 12
    assert sort_ref.count_read(b"@a\nAC\n+\nII\n@tail") == 2 and sort_ref.count_read(b"") == 0 and sort_ref.count_read(b"@a\nAC\n") == 1
    two = b"@b\nAC\n+\nII\n@a\nAC\n+\n55\n@c\nA\n+\nI\n"
    assert sort_ref.simulate(two)[0] == b"@c\nA\n+\nI\n@b\nAC\n+\nII\n@a\nAC\n+\n55\n"      # shorter first, equal keys in input order
    assert sort_ref.simulate(two, by_name=True)[0] == b"@a\nAC\n+\n55\n@b\nAC\n+\nII\n@c\nA\n+\nI\n"
    assert sort_ref.simulate(two, r=None, rewindable=False)[0] == b""
    with pytest.raises(sort_ref.NoAnswer):
        sort_ref.simulate(two, r=2)
    # bytes compare as unsigned, a longer line comes later whatever its bytes
    hi = b"@x\n\xff\n+\nI\n@y\nAA\n+\nII\n@z\nA\n+\nI\n"
    assert [r[0] for r in sort_ref.records(sort_ref.simulate(hi)[0])] == [b"@z", b"@x", b"@y"]
    # the bookkeeping: 6 bytes, then 8 at a time; equal keys leave at once
    keys = [b"ACGTACGTACGTACGTAAAA", b"ACGTACGTACGTACGTAAAC", b"ACGTACTTTT", b"ACGTACTTTT", b"ACGTAC", b"ACGTAC", b"ACGTACGTACTTACGGTTTT"]
    assert sort_ref.refinement(keys) == [3, 2]
    assert sort_ref.refinement([b"A" * 30] * 5) == [] and sort_ref.refinement([]) == []
