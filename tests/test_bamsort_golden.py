"""CPU: the recorded runs of the reference's `samtools sort` (tests/golden/bamsort/manifest.json, made by
tests/golden/make_golden_bamsort.py) against (a) the sequential restatement tests/bamsort_ref.py -- both keys, the stable order,
change_SO, the chunk accounting with its slots that move with the sort, the merge outside the domain, the writer's cuts, zlib at
the recorded level -- and (b) the host sorter bin/bam_sort falls back to (highperformancengs_amd/csrc/host/bam_sort_host.hpp)
inside a stand-alone program with its own main (tests/bamsort_host_main.cpp), built plain and with
g++ -fsanitize=address,undefined and run as a process of its own: nothing built here is loaded into python.  The GPU side of
the same manifest is tests/test_bamsort_gpu.py."""
import base64
import hashlib
import json
import os
import subprocess

import pytest

import bamsort_inputs
import bamsort_ref
from conftest import GOLDEN, PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLDEN, "bamsort", "manifest.json")) as _f:
    MANIFEST = json.load(_f)
CASES = MANIFEST["cases"]
SORTED = [c for c in CASES if c["input"] and c["out"]]


@pytest.fixture(scope="module")
def inputs():
    return bamsort_inputs.own_inputs()


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bamsort_inputs"))
    return d, bamsort_inputs.materialize(d)


def check_bam(case, got):
    """`got`: the output's bytes, or None where none was written"""
    want = case["bam"]
    if want is None:
        assert got is None, case["id"]
        return
    assert got is not None, case["id"]
    assert len(got) == want["size"], case["id"]
    assert hashlib.sha256(got).hexdigest() == want["sha256"], case["id"]
    if want["b64"] is not None:
        assert got == base64.b64decode(want["b64"]), case["id"]


def test_manifest_is_complete():
    ids = {c["id"] for c in CASES}
    assert set(bamsort_inputs.names()) <= ids and {"missing_input", "one_argument", "no_arguments"} <= ids
    assert all(c["expect"] == "same" and c["why"] is None and c["rc"] in (0, 1) for c in CASES)       # the reference finished every case
    assert {c["id"] for c in CASES if c["rc"] == 1} == {"one_argument", "no_arguments"}
    assert all(c["listing"] == ([c["out"]] if c["bam"] and c["out"] != "stdout" else []) for c in CASES)      # no temporary file stays


def test_inputs_are_the_recorded_ones(made):
    assert made[1] == MANIFEST["inputs"]


def test_every_case_has_its_route(inputs):
    """the domain rule puts every case on one of the two lists, and the lists hold what they are there for"""
    for c in CASES:
        assert c["route"] in ("device", "host"), c["id"]
        if c["input"] and "-n" not in c["opts"]:
            assert c["route"] == bamsort_ref.route(inputs[c["input"]]), c["id"]
    by = {c["id"]: c["route"] for c in CASES}
    assert all(by[n] == "host" for n in ("pos_out_2p30m1", "pos_out_m2", "pos_out_2p31m1", "trunc_bytes", "trunc_stream", "strands_n", "tid_below"))
    assert all(by[n] == "device" for n in ("pos_edges_in", "placed_pos_m1", "unplaced_pos", "tid_beyond", "no_eof", "oversize"))


def test_inputs_hold_what_they_are_named_for(inputs):
    recs = bamsort_ref.parse(inputs["residues"]).recs
    out, order = bamsort_ref.sorted_stream(inputs["residues"])
    src, dst, at = {}, {}, 0
    for i, r in enumerate(recs):
        src[i], at = at % 16, at + len(r)
    at = 0
    for j, i in enumerate(order):
        dst[i], at = at % 16, at + len(out[j])
    assert {len(r) % 16 for r in recs} == set(range(16))
    assert {(src[i], dst[i]) for i in range(len(recs))} == {(a, b) for a in range(16) for b in range(16)}
    sizes = {len(r) for r in bamsort_ref.parse(inputs["oversize"]).recs}
    assert {0xff00, 0xff00 + 1, 70000} <= sizes
    fill, _ = bamsort_ref.sorted_stream(inputs["exact_fill"])
    assert len(fill[0]) + len(fill[1]) == 0xff00 and len(fill) == 3
    assert len(bamsort_ref.parse(inputs["hd_long"]).text) > 0xff00
    keys = bamsort_ref.model_keys(bamsort_ref.parse(inputs["all_equal"]).recs)
    assert len(set(keys.tolist())) == 1 and len(keys) == 60
    for n in (1, 2, 3, 255, 256, 257):
        p = bamsort_ref.parse(inputs["targets_%d" % n])
        assert len(p.targets) == n and {n - 1, -1} <= {bamsort_ref.fields(r)[0] for r in p.recs}


@pytest.mark.parametrize("case", SORTED, ids=[c["id"] for c in SORTED])
def test_restatement(case, inputs):
    bam, err = bamsort_ref.sort(inputs[case["input"]], **bamsort_ref.options(case["opts"]))
    assert err == case["stderr"]
    check_bam(case, bam)


def test_the_level_is_ignored_when_merging():
    by = {c["id"]: c for c in CASES}
    assert by["strands_l1_m_3"]["bam"]["sha256"] == by["strands"]["bam"]["sha256"] != by["strands_l1"]["bam"]["sha256"]
    assert by["strands_l0_m_3"]["bam"]["sha256"] == by["strands"]["bam"]["sha256"] != by["strands_l0"]["bam"]["sha256"]


def test_slots_move_with_the_sort(inputs):
    """the file count is not a function of the sizes alone: with the slots left where they were the model gives another number"""
    case = next(c for c in CASES if c["id"] == "strands_m_3")
    recs = bamsort_ref.parse(inputs["strands"]).recs
    sizes, m = [len(r) for r in recs], int(case["opts"][1])
    keys = bamsort_ref.model_keys(recs)
    moved = bamsort_ref.plan_chunks(sizes, m, 1, lambda idx: sorted(idx, key=lambda i: keys[i]))
    still = bamsort_ref.plan_chunks(sizes, m, 1, lambda idx: idx)
    assert case["stderr"] == bamsort_ref.MSG_MERGING % len(moved) and len(still) != len(moved)


def test_change_so():
    so = b"coordinate"
    assert bamsort_ref.change_so(b"", so) == b"@HD\tVN:1.3\tSO:coordinate\n"
    assert bamsort_ref.change_so(b"@HD", so) == b"@HD\tVN:1.3\tSO:coordinate\n@HD"              # three bytes are no @HD line yet
    assert bamsort_ref.change_so(b"@HD\tVN:1.0", so) == b"@HD\tVN:1.0"                           # a line without its end: left alone
    assert bamsort_ref.change_so(b"@HD\tVN:1.0\n@SQ\tSO:x\n", so) == b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSO:x\n"
    assert bamsort_ref.change_so(b"@HD\tSO:coord\n", so) == b"@HD\tSO:coord\n"                   # a prefix at the line's end passes for equal
    assert bamsort_ref.change_so(b"@HD\tSO:coordinates\n", so) == b"@HD\tSO:coordinate\n"
    assert bamsort_ref.change_so(b"@HD\tSO:unsorted\tVN:1\n", so) == b"@HD\tSO:coordinate\tVN:1\n"


def test_strnum_cmp():
    c = bamsort_ref.strnum_cmp
    assert c(b"r9", b"r10") < 0 and c(b"r010", b"r10") < 0 and c(b"r10", b"r10") == 0 and c(b"a", b"b") < 0
    assert c(b"r1x", b"r1") > 0 and c(b"r12", b"r13") < 0 and c(b"r2", b"r") > 0


def build_host(tmp, sanitize):
    exe = os.path.join(tmp, "bamsort_host_san" if sanitize else "bamsort_host")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bamsort_host_main.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("bamsort_host_" + request.param)), request.param == "sanitized")


def test_host_sorter(host_program, made, tmp_path):
    """every recorded case through the stand-alone program: the output byte for byte, stderr, status and what is left behind"""
    for case in CASES:
        work = tmp_path / case["id"]
        work.mkdir()
        if case["input"]:
            os.symlink(bamsort_inputs.path_of(case["input"], made[0]), work / "in.bam")
        p = subprocess.run([host_program] + case["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == case["rc"], (case["id"], p.stderr[-2000:])
        assert p.stderr.decode("latin-1") == case["stderr"], case["id"]
        if case["out"] == "stdout":
            check_bam(case, p.stdout)
        else:
            assert p.stdout == b""
            out = work / case["out"] if case["out"] else None
            check_bam(case, out.read_bytes() if out is not None and out.exists() else None)
        assert sorted(fn for fn in os.listdir(work) if fn != "in.bam") == case["listing"], case["id"]
