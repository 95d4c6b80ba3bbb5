"""CPU: the recorded reference runs of map_kseq (tests/golden/kseq/manifest.json, made by tests/golden/make_golden_kseq.py)
against (a) the Python restatement of kseq_read, the two programs and the route classifier (tests/kseq_ref.py), and (b) the
host parser the tools fall back to (highperformancengs_amd/csrc/host/kseq_read.hpp) inside a stand-alone program with its own
main (tests/kseq_host_main.cpp), built with g++ -fsanitize=address,undefined and run as a process of its own: nothing built here
is loaded into python.  The GPU side of the same manifest is tests/test_kseq_gpu.py."""
import gzip
import hashlib
import json
import os
import subprocess

import pytest

import kseq_inputs
import kseq_ref
from conftest import GOLDEN, PKG

OWN = "kseq/inputs/"


def load_manifest():
    with open(os.path.join(GOLDEN, "kseq", "manifest.json")) as f:
        return json.load(f)


MANIFEST = load_manifest()
CASES = MANIFEST["cases"]
_own = {}


def raw_input(case):
    """the bytes of the case's input file (None: the case has none)"""
    if case["in"] is None:
        return None
    if case["in"].startswith(OWN):
        if not _own:
            _own.update(kseq_inputs.own_inputs())
            for gz, src in kseq_inputs.gz_inputs().items():
                _own[gz] = gzip.compress(_own[src], 6, mtime=0)
        return _own[case["in"][len(OWN):]]
    with open(os.path.join(GOLDEN, case["in"]), "rb") as f:
        return f.read()


def stream(case):
    """the inflated stream of a case that has an answer"""
    raw = raw_input(case)
    if raw is None:
        return b""
    return gzip.decompress(raw) if case["in"].endswith(".gz") else raw


def check_blob(blob, got, what):
    assert len(got) == blob["size"], what
    assert hashlib.sha256(got).hexdigest() == blob["sha256"], what
    if blob["text"] is not None:
        assert got == blob["text"].encode("latin-1"), what


def test_the_inputs_are_the_recorded_ones():
    own = kseq_inputs.own_inputs()
    assert {n: hashlib.sha256(t).hexdigest() for n, t in own.items()} == MANIFEST["inputs"]
    for c in CASES:
        if c["in"] is not None:
            assert hashlib.sha256(raw_input(c)).hexdigest() == c["in_sha256"], c["id"]


def test_the_manifest_covers_both_routes_and_every_expectation():
    same = [c for c in CASES if c["expect"] == "same"]
    assert {c["route"] for c in same} == {"device", "host"}
    assert {c["expect"] for c in CASES} == {"same", "refuse", "usage"}
    assert {c["why"] for c in CASES if c["expect"] == "refuse"} == {"damaged stream", "NUL byte", "mixed lengths"}
    assert all(c["why"] for c in CASES if c["expect"] != "same")


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] == "same"], ids=lambda c: c["id"])
def test_restatement_same(case):
    text = stream(case)
    out, err = kseq_ref.map_kseq(text) if case["tool"] == "map_kseq" else kseq_ref.kbtree_kseq(text)
    check_blob(case["stdout"], out, case["id"])
    assert err == case["stderr"].encode("latin-1")
    assert kseq_ref.route(text) == case["route"]


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] == "refuse"], ids=lambda c: c["id"])
def test_restatement_refuse(case):
    raw = raw_input(case)
    if case["why"] == "damaged stream":
        with pytest.raises(Exception):
            gzip.decompress(raw)
    elif case["why"] == "NUL byte":
        assert b"\0" in stream(case)
    else:
        assert case["tool"] == "kbtree_kseq" and kseq_ref.kbtree_kseq(stream(case)) is None


def test_the_restatement_passes_over_every_second_fasta_header():
    """what a NEW kseq_t per record does to a FASTA file -- the recorded run says so, not only the restatement"""
    case = next(c for c in CASES if c["id"] == "f_fa_passed_over_fa")
    recs = kseq_ref.kseq_records(stream(case))
    assert [r.name for r in recs] == [b"r%d" % i for i in range(0, 11, 2)]
    assert case["stderr"] == "%d\n" % len({r.seq for r in recs})


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kseq_host") / "kseq_host_main")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kseq_host_main.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it runs in whatever environment it is given)
                           "-I", os.path.join(PKG, "csrc"), src, "-o", exe])
    return exe


def run_host(exe, tmp_path, text, *more):
    path = tmp_path / "in"
    path.write_bytes(text)
    return subprocess.run([exe, str(path), *more], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] == "same"], ids=lambda c: c["id"])
def test_host_parser_same(case, host_program, tmp_path):
    p = run_host(host_program, tmp_path, stream(case), *(["btree"] if case["tool"] == "kbtree_kseq" else []))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stderr == case["stderr"].encode("latin-1")      # (a sanitizer's report would stand here)
    check_blob(case["stdout"], p.stdout, case["id"])


@pytest.mark.parametrize("case", [c for c in CASES if c["why"] in ("NUL byte", "mixed lengths")], ids=lambda c: c["id"])
def test_host_parser_refuse(case, host_program, tmp_path):
    text = stream(case)
    p = run_host(host_program, tmp_path, text, *(["btree"] if case["tool"] == "kbtree_kseq" else []))
    assert p.returncode == 2 and p.stdout == b""
    if case["why"] == "mixed lengths":
        assert p.stderr == b"%d %d\n" % tuple(kseq_ref.lengths(text)[:2])
