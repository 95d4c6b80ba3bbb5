"""CPU: the recorded runs of the reference's `samtools merge` (tests/golden/bammerge/manifest.json, made by
tests/golden/make_golden_bammerge.py) against (a) the sequential restatement tests/bammerge_ref.py -- the heap's key, the heap
with its early end at HEAP_EMPTY, the header rule, -h, the level rule, -r, -n, the writer's cuts -- and (b) the host merger
bin/bam_merge falls back to (highperformancengs_amd/csrc/host/bam_merge_host.hpp) inside a stand-alone program with its own main
(tests/bammerge_host_main.cpp), built plain and with g++ -fsanitize=address,undefined and run as a process of its own: nothing
built here is loaded into python.  test_running_maximum_is_the_heap holds the device's formulation -- a stable sort by the
running maximum of the keys inside every file -- to the restated heap.  The GPU side of the same manifest is
tests/test_bammerge_gpu.py."""
import base64
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bammerge_inputs
import bammerge_ref
from conftest import GOLDEN, PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLDEN, "bammerge", "manifest.json")) as _f:
    MANIFEST = json.load(_f)
CASES = MANIFEST["cases"]
MERGED = [c for c in CASES if len(c["args"]) - len(c["opts"]) >= 3]
OLD = b"what was here before\n"


@pytest.fixture(scope="module")
def sets():
    return bammerge_inputs.own_sets()


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


def lay_out(case, sets, work):
    """the case's directory as the recorder made it; returns the names that are not output"""
    given = bammerge_inputs.materialize(str(work), case["set"], sets[case["set"]]) if case["set"] else []
    if case["h"]:
        (work / "h.sam").write_text(bammerge_inputs.header_files()[case["h"]])
        given.append("h.sam")
    if case["old"]:
        (work / "out.bam").write_bytes(OLD)
    return given


def check_run(case, p, work, given):
    assert p.returncode == case["rc"], (case["id"], p.stderr[-2000:])
    if case["out"] == "stdout":
        check_bam(case, p.stdout)
    else:
        assert p.stdout == b""
        out = work / "out.bam"
        check_bam(case, out.read_bytes() if out.exists() else None)
    assert sorted(fn for fn in os.listdir(work) if fn not in given) == case["listing"], case["id"]


def test_manifest_is_complete():
    ids = {c["id"] for c in CASES}
    assert set(bammerge_inputs.names()) <= ids
    assert {"missing_input", "missing_first", "two_arguments", "no_arguments", "three_sorted_exists", "three_sorted_f_over", "three_sorted_stdout",
            "two_sorted_h_match", "two_sorted_h_count", "two_sorted_h_name", "two_sorted_h_missing", "rg_tagged_r", "names_n"} <= ids
    assert {"l0", "l1", "l9", "l12", "u", "1", "u_1_l9", "t2", "f", "n", "r"} <= {i[len("three_sorted_"):] for i in ids if i.startswith("three_sorted_")}
    assert all(c["expect"] == "same" and c["why"] is None and c["rc"] in (0, 1) for c in CASES)       # the reference finished every case
    assert all(c["listing"] == (["out.bam"] if c["bam"] and c["out"] != "stdout" else []) for c in CASES)
    assert {c["id"] for c in CASES if c["rc"] == 1} == {"name_mismatch", "three_sorted_exists", "two_sorted_h_count", "two_sorted_h_name",
                                                         "two_sorted_h_missing", "more_targets_h_count", "missing_input", "missing_first",
                                                         "two_arguments", "no_arguments"}


def test_inputs_are_the_recorded_ones():
    assert bammerge_inputs.digests() == MANIFEST["inputs"]
    assert {k: hashlib.sha256(v.encode()).hexdigest() for k, v in bammerge_inputs.header_files().items()} == MANIFEST["headers"]


def test_inputs_hold_what_they_are_named_for(sets):
    recs = lambda name: [bammerge_ref.parse(f).recs for f in sets[name]]
    keys = lambda name: [[bammerge_ref.key(r) for r in f] for f in recs(name)]
    is_sorted = lambda k: all(a <= b for a, b in zip(k, k[1:]))
    for name in ("two_sorted", "three_sorted", "seventeen", "pos_wide", "pos_high", "residues"):
        assert all(is_sorted(k) for k in keys(name)), name
    assert len(sets["seventeen"]) == 17
    assert [len(f) for f in recs("empty_first")][0] == 0 and [len(f) for f in recs("empty_middle")][1] == 0 and [len(f) for f in recs("empty_last")][2] == 0
    assert len(recs("one_record")[1]) == 1
    assert len({k for f in keys("equal_keys") for k in f} & set(keys("equal_keys")[0])) and all(bammerge_ref.key(r) in keys("equal_keys")[1] for r in recs("equal_keys")[0][1:6])
    assert all({k & 1 for k in f} == {0, 1} and len({k >> 1 for k in f}) == 1 for f in keys("both_strands"))
    for name in ("heap_empty_m2", "heap_empty_2p31m2", "heap_empty_mid"):
        assert any(bammerge_ref.EMPTY in k for k in keys(name)), name
    wide = {bammerge_ref.fields(r)[1] for f in recs("pos_wide") for r in f}
    assert {(1 << 30) - 1, (1 << 31) - 1, -2} <= wide and not any(bammerge_ref.EMPTY in k for k in keys("pos_wide"))
    high = {bammerge_ref.fields(r)[1] for f in recs("pos_high") for r in f}
    assert {(1 << 30) - 1, (1 << 31) - 1, (1 << 31) - 2} <= high and min(high) == -1 and not any(bammerge_ref.EMPTY in k for k in keys("pos_high"))
    first = keys("unsorted_first_largest")[0]
    assert first[0] == max(first) and is_sorted(first[1:])
    down = keys("unsorted_descending")[0]
    assert all(a >= b for a, b in zip(down, down[1:])) and down[0] > down[-1]
    mid = keys("unsorted_unmapped_mid")[0]
    assert mid[20] >> 32 == 0xffffffff and mid[21] >> 32 != 0xffffffff
    assert [len(bammerge_ref.parse(f).targets) for f in sets["more_targets_later"]] == [3, 5, 4]
    assert len(bammerge_ref.parse(sets["hd_long"][0]).text) > 0xff00
    assert not bammerge_ref.parse(sets["hd_none"][0]).text.startswith(b"@HD")
    assert {len(r) % 16 for f in recs("residues") for r in f} == set(range(16))
    assert {0xff00, 0xff00 + 1, 70000} <= {len(r) for f in recs("oversize") for r in f}
    assert sum(len(f) for f in recs("residues")) > 1000


@pytest.mark.parametrize("case", MERGED, ids=[c["id"] for c in MERGED])
def test_restatement(case, sets):
    if case["old"] and "-f" not in case["opts"]:
        got = (OLD, bammerge_ref.MSG_EXISTS % "out.bam", 1)
    else:
        given = case["args"][len(case["opts"]) + 1:]
        on_disk = {"in%d.bam" % (k + 1): f for k, f in enumerate(sets[case["set"]])}
        kw = bammerge_ref.options(case["opts"])
        if "h_name" in kw:
            kw["h_text"] = bammerge_inputs.header_files()[case["h"]].encode() if case["h"] else None
        got = bammerge_ref.merge([on_disk.get(os.path.basename(g)) for g in given], given, **kw)
    assert got[1] == case["stderr"] and got[2] == case["rc"]
    check_bam(case, got[0])


def test_the_level_options_change_no_byte():
    """bam_merge_core2 opens its output with the literal "w": -u, -1, -l and -@ leave the recorded output as it is"""
    by = {c["id"]: c for c in CASES}
    for k in ("l0", "l1", "l9", "l12", "l_neg", "u", "1", "u_1_l9", "1_l9", "t2", "u_t2", "f", "f_over", "stdout", "stdout_u"):
        assert by["three_sorted_" + k]["bam"]["sha256"] == by["three_sorted"]["bam"]["sha256"], k


def test_running_maximum_is_the_heap():
    """2,000 seeded random file sets, sorted or not: a stable sort of the records, file after file, by the running maximum of the
    keys inside their file is the order the restated heap writes -- and the count of lifted records is 0 exactly for sorted files"""
    rs = np.random.RandomState(20240)
    for trial in range(2000):
        n_files = int(rs.randint(2, 6))
        span = int(rs.choice([2, 5, 40]))
        keys = [[int(k) for k in rs.randint(0, span, int(rs.randint(0, 8)))] for _ in range(n_files)]
        if trial % 4 == 0:
            keys = [sorted(k) for k in keys]
        order, lifted = bammerge_ref.effective_order(keys)
        assert order == bammerge_ref.heap_order(keys), (trial, keys)
        assert (lifted == 0) == all(a <= b for k in keys for a, b in zip(k, k[1:])), (trial, keys)


def test_every_case_has_its_route(sets):
    """the domain rule puts every case on one of the two lists, and the lists hold what they are there for"""
    for c in CASES:
        assert c["route"] in ("device", "host"), c["id"]
        if c["set"] and c["rc"] == 0:
            assert c["route"] == bammerge_ref.route(sets[c["set"]], c["opts"]), c["id"]
        else:
            assert c["route"] == "host", c["id"]
    by = {c["id"]: c["route"] for c in CASES}
    assert all(by[n] == "host" for n in ("heap_empty_m2", "heap_empty_2p31m2", "heap_empty_mid", "names_n", "rg_tagged_r", "three_sorted_nr_u", "name_mismatch",
                                         "pos_wide"))      # (pos -2 has its key in the heap, but the record index takes no pos below -1)
    assert all(by[n] == "device" for n in ("pos_high", "unplaced_pos", "placed_pos_m1", "unsorted_all", "unsorted_descending", "seventeen", "no_eof",
                                           "oversize", "two_sorted_h_match", "more_targets_later", "all_empty"))


def test_rg_edit():
    import struct
    from bai_inputs import rec
    r = rec(0, 5, "10M", 0, "x", aux=b"NMC\x01RGZold\0XSA+")
    out = bammerge_ref.rg_edit(r, b"in1")
    assert out.endswith(b"NMC\x01XSA+RGZin1\0") and struct.unpack_from("<i", out)[0] == len(out) - 4
    assert bammerge_ref.rg_edit(rec(0, 5, "10M", 0, "x"), b"f").endswith(b"RGZf\0")
    assert bammerge_ref.rg_name("dir/sub/lane1.bam") == b"lane1" and bammerge_ref.rg_name(".bam") == b".bam" and bammerge_ref.rg_name("a.sam") == b"a.sam"


def build_host(tmp, sanitize):
    exe = os.path.join(tmp, "bammerge_host_san" if sanitize else "bammerge_host")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bammerge_host_main.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("bammerge_host_" + request.param)), request.param == "sanitized")


def test_host_merger(host_program, sets, tmp_path):
    """every recorded case through the stand-alone program: the output byte for byte, stderr, status and what is left behind"""
    for case in CASES:
        work = tmp_path / case["id"]
        work.mkdir()
        given = lay_out(case, sets, work)
        p = subprocess.run([host_program] + case["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.stderr.decode("latin-1") == case["stderr"], case["id"]
        check_run(case, p, work, given)


def test_region_option_is_refused(host_program, sets, tmp_path):
    """-R is out of scope: the tool says so and leaves with status 2 before it touches the output"""
    given = bammerge_inputs.materialize(str(tmp_path), "two_sorted", sets["two_sorted"])
    p = subprocess.run([host_program, "-R", "c0:1-100", "out.bam"] + given, cwd=tmp_path, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"-R" in p.stderr and b"not supported" in p.stderr and p.stdout == b""
    assert sorted(os.listdir(tmp_path)) == sorted(given)


def test_outside_the_domain_is_said(host_program, sets, tmp_path):
    """where the reference crashes or never ends the tool leaves with status 2 and a reason: an input cut inside a record behind
    its first one, -n with an input of no records, an input that is no BAM file"""
    a, b = sets["two_sorted"]
    (tmp_path / "in1.bam").write_bytes(a)
    (tmp_path / "in2.bam").write_bytes(b)
    whole = bammerge_ref.parse(b)
    from bai_inputs import bgzf, header, refs
    stream = header(refs(3)) + b"".join(whole.recs)
    (tmp_path / "cut.bam").write_bytes(bgzf([stream[:len(stream) - 17]]))
    (tmp_path / "empty.bam").write_bytes(sets["all_empty"][0])
    (tmp_path / "text.bam").write_bytes(b"not a BAM file\n")
    for args, word in ((["out.bam", "in1.bam", "cut.bam"], b"ends inside a record"), (["-n", "out.bam", "in1.bam", "empty.bam"], b"holds no record"),
                       (["out.bam", "in1.bam", "text.bam"], b"no BAM file")):
        p = subprocess.run([host_program, "-f"] + args, cwd=tmp_path, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2 and word in p.stderr and b"outside the tool's domain" in p.stderr, (args, p.stderr)
