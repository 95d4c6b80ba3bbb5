"""CPU: the Python restatement of pick_pair (pair_ref.py: the framing, the walk, and the propose-and-verify procedure as plain
loops) equals every output and stderr line recorded from the compiled reference (tests/golden/pair/), has no answer where the
reference has none, and every pairing its certificate accepts is the walk's."""
import atexit
import gzip
import hashlib
import json
import os
import shutil
import tempfile
import zlib

import numpy as np
import pytest

import pair_inputs
import pair_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "pair", "manifest.json")))
CASES = MANIFEST["cases"]
BY_ID = {c["id"]: c for c in CASES}
OWN = pair_inputs.OWN
SUFFIXES = ("_1_PE.fq.gz", "_1_SE.fq.gz", "_2_PE.fq.gz", "_2_SE.fq.gz")
_made = []


def input_path(rel):
    """A case's input file: a file of tests/golden/fastq/, or one of tests/pair_inputs.py -- those are made once per process in a
    temporary directory and held to the digests the recorder stored."""
    if not rel.startswith(OWN):
        return os.path.join(GOLDEN, rel)
    if not _made:
        _made.append(tempfile.mkdtemp(prefix="pair_inputs_"))
        atexit.register(shutil.rmtree, _made[0], ignore_errors=True)
        pair_inputs.materialize(_made[0], MANIFEST["inputs"])
    return os.path.join(_made[0], rel[len(OWN):])


def read_input(rel):
    raw = open(input_path(rel), "rb").read()
    return gzip.decompress(raw) if rel.endswith(".gz") else raw


def prefix(case):
    """The outputs' prefix: the last of -1 and -o on the command line."""
    p = "out"
    for i, a in enumerate(case["args"][:-1]):
        if a in ("-1", "-o"):
            p = case["args"][i + 1]
    return p


def expected(case):
    """({file name: inflated bytes}, stderr) of a case the reference answers, from the restatement."""
    outs, err = pair_ref.run(read_input(case["a"]), read_input(case["b"]))
    return {prefix(case) + s: o for s, o in zip(SUFFIXES, outs)}, err


def check_blob(o, text, what):
    assert len(text) == o["size"], what
    assert hashlib.sha256(text).hexdigest() == o["sha256"], what
    if o["text"] is not None:
        assert text == o["text"].encode("latin-1"), what


def check_outputs(case, files):
    """files: {file name: inflated bytes}.  Everything the reference wrote equals them."""
    assert sorted(files) == sorted(o["name"] for o in case["outputs"]), case["id"]
    for o in case["outputs"]:
        check_blob(o, files[o["name"]], case["id"] + " " + o["name"])


SAME = [c for c in CASES if c["expect"] == "same"]
REFUSE = [c for c in CASES if c["expect"] == "refuse"]
DAMAGED = [c for c in CASES if c["expect"] == "damaged"]
ids = lambda cs: [c["id"] for c in cs]


@pytest.mark.parametrize("case", SAME, ids=ids(SAME))
def test_restatement_equals_the_reference(case):
    files, err = expected(case)
    check_outputs(case, files)
    assert err == case["stderr"]


@pytest.mark.parametrize("case", REFUSE, ids=ids(REFUSE))
def test_restatement_has_no_answer_where_the_reference_crashes(case):
    with pytest.raises(pair_ref.NoAnswer):
        expected(case)


@pytest.mark.parametrize("case", DAMAGED, ids=ids(DAMAGED))
def test_damaged_inputs_are_damaged(case):
    with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
        read_input(case["a"])


@pytest.mark.parametrize("case", SAME + REFUSE, ids=ids(SAME + REFUSE))
def test_the_stated_route_is_the_certificates_and_what_it_accepts_is_the_walk(case):
    a, b = read_input(case["a"]), read_input(case["b"])
    assert pair_ref.predicted_route(a, b) == case["route"] == next(c for c in pair_inputs.cases() if c["id"] == case["id"])["route"]
    if case["route"] != "host":
        assert case["expect"] == "same"
        assert pair_ref.device(a, b)[1] == pair_ref.walk(a, b)


def test_every_fixture_reproduces_its_recorded_hash():
    digest = lambda rel: hashlib.sha256(open(input_path(rel), "rb").read()).hexdigest()
    n = 0
    for c in CASES:
        for side in ("a", "b"):
            if c[side]:
                assert digest(c[side]) == c[side + "_sha256"], (c["id"], side)
                n += 1
    assert n >= 140 and sorted(MANIFEST["inputs"]) == sorted(pair_inputs.own_inputs())


def test_the_goldens_cover_what_they_claim():
    assert [c["id"] for c in CASES] == [c["id"] for c in pair_inputs.cases()]
    assert len(SAME) >= 60 and all(c["rc"] == 0 for c in SAME) and all(c["rc"] == -11 for c in REFUSE)
    # the device route serves at least two thirds of the cases the reference answers, and both proposals are there
    routes = [c["route"] for c in SAME]
    assert 3 * (routes.count("identity") + routes.count("join")) >= 2 * len(SAME)
    assert routes.count("identity") >= 20 and routes.count("join") >= 20 and routes.count("host") >= 5
    # the crashes of the walk
    assert {c["id"] for c in REFUSE} >= {"a_empty", "b_empty", "a_runs_out", "one_side_left", "b_left", "unsorted_gap", "trunc_b", "self_trunc_fq"}
    out = lambda cid, k: next(o for o in BY_ID[cid]["outputs"] if o["name"].endswith(SUFFIXES[k]))
    # the mispair: @b goes with @c; the prefix match: @r1 with @r10; the lone tail record; two empty files
    assert out("mispair", 0)["text"].startswith("@b 1\n") and out("mispair", 2)["text"].startswith("@c 2\n") and out("mispair", 3)["text"].startswith("@a 2\n")
    assert out("prefix", 2)["text"].startswith("@r10 2\n") and out("prefix", 1)["size"] == 0
    assert out("tail", 0)["text"].startswith("@e 1\n") and out("tail", 2)["size"] == 0 and out("tail", 3)["size"] == 58
    assert [out("both_empty", k)["size"] for k in range(4)] == [0, 0, 0, 0]
    # a name without a space is compared whole: @q1 is no mate of @q1/2, but "@q1 1" is one of "@q1"
    assert out("nospace_longer_b", 1)["text"].startswith("@q1\n") and out("nospace_in_b", 1)["size"] == 0
    # a last record without its newline goes out without one; CRLF stays
    assert not out("nonl_both", 0)["text"].endswith("\n") and out("nonl_a", 2)["text"].endswith("\n")
    assert out("crlf", 0)["text"].count("\r\n") == 3 * 3 and "\n+\n" in out("crlf", 0)["text"]
    # -1 sets the prefix: an -o in front of it is lost
    assert {o["name"] for o in BY_ID["o_before_1"]["outputs"]} == {"a.fq" + s for s in SUFFIXES}
    assert {o["name"] for o in BY_ID["o_twice"]["outputs"]} == {"z" + s for s in SUFFIXES}
    assert {o["name"] for o in BY_ID["only_1_and_2"]["outputs"]} == {"a.fq" + s for s in SUFFIXES}
    for cid, name in (("missing_1", "no_such_file.fq"), ("missing_2", "no_such_file.fq")):
        assert BY_ID[cid]["expect"] == "missing" and BY_ID[cid]["rc"] == 1 and BY_ID[cid]["stderr"] == "open file %s failed\n" % name
    assert all(BY_ID[u]["expect"] == "usage" and BY_ID[u]["rc"] == 1 for u in ("no_arguments", "help", "unknown_option"))


def random_names(rs, n):
    """Small alphabets and lengths, so that prefixes, duplicates, names without a space and bytes >= 0x80 all happen."""
    out = []
    for _ in range(n):
        stem = bytes(rs.choice(np.frombuffer(b"ab\xe9", np.uint8), rs.randint(1, 4)))
        out.append(b"@" + stem + (b" %d" % rs.randint(0, 3) if rs.randint(0, 4) else b""))
    return out


def test_the_certificate_is_sound_on_random_inputs():
    """Whatever the proposals are, a pairing that passes V1 .. V5 is the walk's partition; and mangled proposals do not pass."""
    rs = np.random.RandomState(77)
    accepted = rejected = 0
    for trial in range(4000):
        na, nb = random_names(rs, rs.randint(0, 7)), random_names(rs, rs.randint(0, 7))
        if trial % 2:
            na, nb = sorted(na), sorted(nb)
        if trial % 4 >= 2:      # B as A's mates with reads lost on either side
            nb = [n for n in na if rs.randint(0, 4)]
            na = [n for n in na if rs.randint(0, 4)]
        a, b = pair_inputs.named(na, nb)
        try:
            walked = pair_ref.walk(a, b)
        except pair_ref.NoAnswer:
            walked = None
        proposals = [pair_ref.propose_identity(na, nb), pair_ref.propose_join(na, nb),
                     [int(j) if j < len(nb) else None for j in rs.randint(0, len(nb) + 2, len(na))]]
        for m in proposals:
            if m is None:
                continue
            if pair_ref.certify(na, nb, m) is None:
                if not na and not nb:
                    continue
                assert walked is not None and pair_ref.partition_of(m, len(nb)) == walked, (na, nb, m)
                accepted += 1
            else:
                rejected += 1
        route, part = pair_ref.device(a, b)
        assert route == "host" or part == walked
    assert accepted >= 300 and rejected >= 300


def test_restatement_units():
    c = pair_ref.compare
    assert c(b"@r1 x", b"@r10 y") == 0 and c(b"@r10 x", b"@r1 y") > 0          # only a's k bytes count; b ends in NUL inside them
    assert c(b"@q1", b"@q1") == 0 and c(b"@q1", b"@q1/2") < 0 and c(b"@q1/2", b"@q1") > 0
    assert c(b"@\xe9 1", b"@z 1") > 0                                           # unsigned bytes
    assert c(b"@a\r", b"@a") > 0 and c(b" x", b"anything") == 0                 # a CRLF name keeps its \r; k = 0 compares nothing
    assert pair_ref.records(b"@a\nAC\n+\nII") == [(b"@a", b"AC", b"II")] and pair_ref.records(b"@a\nAC\n+\nII\n@b") == [(b"@a", b"AC", b"II\n")]
    assert pair_ref.regular(b"@a\nAC\n+\nII\n@b") and not pair_ref.regular(b"@a\nAC\n+\n") and not pair_ref.regular(b"@a\nA\0\n+\nII\n")
    assert pair_ref.regular(b"@" + b"n" * 1021 + b"\nA\n+\nI\n") and not pair_ref.regular(b"@" + b"n" * 1022 + b"\nA\n+\nI\n")
    outs, _ = pair_ref.run(*pair_inputs.named([b"@b 1", b"@e 1"], [b"@a 2", b"@c 2", b"@e 2"]))
    assert [o.count(b"\n+\n") for o in outs] == [2, 0, 2, 1]
    with pytest.raises(pair_ref.NoAnswer):
        pair_ref.walk(*pair_inputs.named([b"@a 1", b"@b 1"], [b"@a 2"]))
