"""CPU: the recorded runs of the reference's `samtools index` (tests/golden/bai/manifest.json, made by
tests/golden/make_golden_bai.py) against (a) the sequential restatement tests/bai_ref.py -- virtual offsets, chunk runs, the
merge, the linear index, the metadata bin, the order of the bins -- and (b) the host indexer bin/bam_index falls back to
(highperformancengs_amd/csrc/host/bai_build.hpp) inside a stand-alone program with its own main (tests/bai_host_main.cpp),
built plain and with g++ -fsanitize=address,undefined and run as a process of its own: nothing built here is loaded into
python.  The GPU side of the same manifest is tests/test_bai_gpu.py."""
import base64
import hashlib
import json
import os
import subprocess

import pytest

import bai_inputs
import bai_ref
from conftest import GOLDEN, PKG

with open(os.path.join(GOLDEN, "bai", "manifest.json")) as _f:
    MANIFEST = json.load(_f)
CASES = MANIFEST["cases"]
WITH_INPUT = [c for c in CASES if c["input"]]


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bai_inputs"))
    return d, bai_inputs.materialize(d)


def check_bai(case, got):
    """`got`: the index's bytes, or None where none was written"""
    want = case["bai"]
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
    assert set(bai_inputs.names()) | {"explicit_out", "missing_input", "no_arguments"} == ids
    assert all(c["expect"] == "same" and c["why"] is None and c["rc"] in (0, 1) for c in CASES)       # the reference finished every case
    assert {c["id"] for c in CASES if c["rc"] == 1} == {"no_arguments"}


def test_inputs_are_the_recorded_ones(made):
    assert made[1] == MANIFEST["inputs"]


def test_committed_indexes_are_not_samtools(made):
    """why the tool exists: the .bai files beside the fixtures come from the test helpers and differ from the reference's"""
    for name in bai_inputs.FIXTURES:
        case = next(c for c in CASES if c["id"] == name)
        committed = open(bai_inputs.path_of(name, made[0]) + ".bai", "rb").read()
        assert len(committed) != case["bai"]["size"]


@pytest.mark.parametrize("case", WITH_INPUT, ids=[c["id"] for c in WITH_INPUT])
def test_restatement(case, made):
    data = open(bai_inputs.path_of(case["input"], made[0]), "rb").read()
    bai, err = bai_ref.index(data)
    assert err == case["stderr"]
    check_bai(case, bai)


def test_bin_order_steps():
    """the table's sizes and where it grows: n buckets hold int(0.77 n + 0.5) keys -- 2, 8, 18, 41, 75, 149, 300, 592 -- before the
    next prime is taken"""
    t = bai_ref.KhOrder()
    sizes = {}
    for k in range(600):
        t.put(7 * k + 1)
        sizes.setdefault(t.n, k + 1)
    assert sizes == {3: 1, 11: 3, 23: 9, 53: 19, 97: 42, 193: 76, 389: 150, 769: 301, 1543: 593}
    assert sorted(t.order()) == [7 * k + 1 for k in range(600)]
    u = bai_ref.KhOrder()
    for key in (5, 16, 27):                  # equal modulo 11.  Three buckets: 5 -> 2, 16 -> 1.  Grown to 11 in slot order: 16 -> 5, then 5 -> 5
        u.put(key)                           # taken, step 1 + 5 % 10 -> 0; 27 -> 5 taken, step 1 + 27 % 10 -> 2
    assert u.order() == [5, 27, 16] and not u.put(16)


def build_host(tmp, sanitize):
    exe = os.path.join(tmp, "bai_host_san" if sanitize else "bai_host")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bai_host_main.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(PKG, "csrc"), src, "-o", exe, "-lz"])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("bai_host_" + request.param)), request.param == "sanitized")


def test_host_indexer(host_program, made, tmp_path):
    """every recorded case through the stand-alone program: the index byte for byte, stderr and status"""
    for case in CASES:
        work = tmp_path / case["id"]
        work.mkdir()
        if case["input"]:
            os.symlink(bai_inputs.path_of(case["input"], made[0]), work / "in.bam")
        p = subprocess.run([host_program] + case["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == case["rc"], (case["id"], p.stderr[-2000:])
        assert p.stdout == b""
        assert p.stderr.decode("latin-1") == case["stderr"], case["id"]
        out = work / case["out"] if case["out"] else None
        check_bai(case, out.read_bytes() if out is not None and out.exists() else None)
        assert sorted(os.listdir(work)) == sorted(({"in.bam"} if case["input"] else set()) | ({case["out"]} if case["bai"] else set()))
