"""CPU: the recorded runs of the reference's `samtools fixmate` (tests/golden/fixmate/manifest.json, made by
tests/golden/make_golden_fixmate.py) against (a) the sequential restatement tests/fixmate_ref.py -- bam_mating_core's loop,
bam_calend, the CT field, the writer's cuts -- and (b) the sequential route bin/bam_fixmate falls back to
(highperformancengs_amd/csrc/host/bam_fixmate_host.hpp) inside a stand-alone program with its own main
(tests/fixmate_host_main.cpp), built plain and with g++ -fsanitize=address,undefined and run as a process of its own: nothing
sanitized is loaded into Python.  (c) The device's closed forms -- pairing as a parity inside runs of equal names, the output's
order as a scan of what every record makes the reference write -- against the loop on seeded random sequences.  The tool on the
device and the hpn_bam_fixmate_* ABI: tests/test_fixmate_gpu.py."""
import base64
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import fixmate_inputs
import fixmate_ref
from conftest import GOLDEN, PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLDEN, "fixmate", "manifest.json")) as _f:
    MANIFEST = json.load(_f)
CASES = MANIFEST["cases"]
UNDEFINED = {"op_eleven_carried", "tid_beyond_header"}


@pytest.fixture(scope="module")
def inputs():
    return fixmate_inputs.own_inputs()


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


def run_case(exe, case, inputs, work, env=None, on_exit=None):
    """one recorded case through a program with fixmate's arguments: the output byte for byte, stderr, status, what is left behind;
    where the reference's run was not recorded (`refuse`): status 2, a reason under [hpn], no output.  on_exit(status, stderr)
    is called before anything is checked.  -> stderr"""
    work.mkdir()
    data = inputs[case["input"]] if case["input"] else None
    given = [fixmate_inputs.materialize(str(work), case["input"], data)] if case["input"] else []
    feed = {"input": data} if case["stdin"] else {"stdin": subprocess.DEVNULL}
    p = subprocess.run([exe] + case["args"], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env, **feed)
    err = p.stderr.decode("latin-1")
    if on_exit:
        on_exit(p.returncode, err)
    said = "".join(l + "\n" for l in err.splitlines() if not l.startswith("[hpn]"))
    if case["expect"] == "refuse":
        assert p.returncode == 2 and "[hpn] bam_fixmate:" in err and p.stdout == b"", (case["id"], p.returncode, err[-2000:])
        assert sorted(os.listdir(work)) == sorted(given), case["id"]
        return err
    assert p.returncode == case["rc"], (case["id"], p.returncode, err[-2000:])
    assert said == case["stderr"], case["id"]
    if case["out"] == "stdout":
        check_bam(case, p.stdout)
    else:
        assert p.stdout == b""
        out = work / "out.bam"
        check_bam(case, out.read_bytes() if out.exists() else None)
    assert sorted(fn for fn in os.listdir(work) if fn not in given) == case["listing"], case["id"]
    return err


def test_manifest_is_complete():
    ids = {c["id"] for c in CASES}
    assert set(fixmate_inputs.names()) <= ids and {n + "_r" for n in fixmate_inputs.names()} <= ids      # every input with and without -r
    assert {"mixed_stdout", "mixed_stdin", "mixed_pipe_r", "one_argument", "one_argument_r", "no_arguments", "missing_input"} <= ids
    refused = {c["id"] for c in CASES if c["expect"] == "refuse"}
    assert refused == {n + s for n in UNDEFINED for s in ("", "_r")} | {"missing_input"}
    assert all(c["rc"] in (0, 1) and c["why"] is None for c in CASES if c["id"] not in refused)
    assert {c["id"] for c in CASES if c["rc"] == 1} == {"one_argument", "one_argument_r", "no_arguments"}
    assert {c["input"] for c in CASES if c["route"] == "host" and c["rc"] == 0 and not c["stdin"] and c["out"] == "out.bam"} == {
        "op_back", "op_ten", "op_ten_not_carried", "name_nul_inside"}


def test_inputs_are_the_recorded_ones_and_hold_what_they_are_named_for(inputs):
    assert fixmate_inputs.digests() == MANIFEST["inputs"]
    recs = lambda n: fixmate_ref.parse(inputs[n]).recs
    tl = lambda n: [ln for _, ln in fixmate_ref.parse(inputs[n]).targets]
    run = lambda n: fixmate_ref.machine(recs(n), tl(n), False)
    ct = lambda n: [r[r.rindex(b"CTZ") + 3:-1] for _, r in run(n)[0] if b"CTZ" in r[36:] and not r.endswith(b"NMC\x01")]
    # a run of equal names one longer than the scan's tile, in front of and behind other records
    names = [fixmate_ref.qname(r) for r in recs("run_past_tile")]
    assert names.count(b"same") == fixmate_inputs.SCAN_TILE + 1 and names[0] == b"lead" and names[-1] == b"tail"
    in_runs = [fixmate_ref.qname(r) for r in recs("run_lengths")]
    assert sorted({in_runs.count(b"run%d" % k) for k in range(11)}) == [1, 2, 3, 4, 5]
    # the order is a permutation: skipped records overtake a pending one
    out, _ = run("skipped_between")
    assert [i for i, _ in out] != sorted(i for i, _ in out)
    assert [i for i, _ in run("mixed")[0]] != list(range(len(recs("mixed"))))
    # ends: a pending record is written as it came
    out, n = run("ends_pending")
    assert out[-1][1] == recs("ends_pending")[out[-1][0]] and struct.unpack_from("<iii", out[-1][1], 24) == (2, 9, 44)
    assert run("ends_pair")[0][-1][0] == len(recs("ends_pair")) - 1 and run("ends_pair")[1]["pairs"] == 1
    assert run("no_records")[0] == [] and run("only_skipped")[1] == {"pairs": 0, "singletons": 0, "tags": 0, "added": 0}
    # the CT text: a tie goes to the earlier record, a swap to the later one, a negative gap, digit counts, no CIGAR at all
    texts = ct("ct_text")
    assert b"1F10M-10T2R12M" in texts and b"2R12M788T1F10M" in texts and b"1F50M-45T2R20M" in texts
    assert b"1F1M9I10M99D100M5S18790T2R7H12345N6=8X3P" in texts and b"1F20T2R" in texts and b"1F20T2R5M" in texts and b"1F0M0T2R0M" in texts
    assert max(len(t) for t in texts) > 0xff00 * 2          # a long CIGAR: the grown record is longer than one block
    assert sum(1 for _, r in run("ct_text")[0] if r.count(b"CTZ") == 2) == 1      # a CT that is there already is not looked for
    assert any(b"268435455M" in t and b"268435455N" in t and b"T" in t and b"-" in t for t in ct("ct_oplen_max"))
    # flags: the end beyond the target sets 0x4, on a live and on a secondary record
    out = dict(run("flags_and_ends")[0])
    src = recs("flags_and_ends")
    flag = lambda r: struct.unpack_from("<H", r, 18)[0]
    assert flag(src[0]) == 0x41 and flag(out[0]) & 0x4 and flag(out[1]) & 0x8 and flag(src[2]) == 0x100 and flag(out[2]) == 0x104 and flag(out[3]) == 0x100
    assert struct.unpack_from("<i", out[0], 32)[0] == 0
    # the emitter: the carrier fits the open block as stored and not with its field
    rs = recs("ct_straddles_cut")
    k = next(i for i, r in enumerate(rs) if fixmate_ref.qname(r) == b"edge")
    assert sum(len(r) for r in rs[:k + 1]) <= fixmate_inputs.FULL < sum(len(r) for r in rs[:k + 1]) + 19
    o = [i for i, _ in run("slice_between_halves")[0]]
    assert fixmate_ref.qname(recs("slice_between_halves")[o[999]]) == fixmate_ref.qname(recs("slice_between_halves")[o[1000]])
    assert max(len(r) for _, r in run("grown_past_block")[0]) > fixmate_inputs.FULL


def test_restatement(inputs):
    """the restatement against every recorded run the reference finished"""
    for case in CASES:
        if case["expect"] != "same" or case["out"] is None:
            continue
        got, err, rc = fixmate_ref.fixmate(inputs[case["input"]], "-r" in case["args"])
        assert rc == case["rc"], case["id"]
        assert (fixmate_ref.MSG_NO_EOF if case["stdin"] else err) == case["stderr"], case["id"]
        check_bam(case, got)
    for name in UNDEFINED:
        assert fixmate_ref.fixmate(inputs[name]) == (None, None, 2)


def test_routes(inputs):
    for case in CASES:
        if case["expect"] == "same" and case["rc"] == 0 and not case["stdin"] and case["out"] == "out.bam":
            assert case["route"] == fixmate_ref.route(inputs[case["input"]]), case["id"]


def test_op_ten_writes_the_strings_nul(inputs):
    """BAM_CIGAR_STR[10] is the string's NUL: the reference writes it into the CT text and counts it (recorded: op_ten)"""
    out, n = fixmate_ref.machine(fixmate_ref.parse(inputs["op_ten"]).recs, [1 << 20] * 3, False)
    assert out[0][1].endswith(b"CTZ1F10M3\x005M185T2R30M\0") and n["tags"] == 1


def test_closed_forms_are_the_state_machine():
    """parity pairing and the write-count order against bam_mating_core's loop: 3,000 seeded random sequences of flags, names and
    refIDs, with and without -r"""
    rs = np.random.RandomState(20261021)
    for trial in range(3000):
        n = int(rs.randint(0, 40))
        n_names = int(rs.randint(1, 6))
        recs = []
        for _ in range(n):
            kind = rs.randint(0, 8)
            tid = -1 if kind == 0 else int(rs.randint(0, 3))
            flag = (0x100 if kind == 1 else 0) | int(rs.randint(0, 2)) | (0x10 if rs.randint(0, 2) else 0) | (0x40 if rs.randint(0, 2) else 0x80)
            pos = int(rs.randint(0, 2000)) if kind != 2 else 999990          # (kind 2: the end lies beyond the target, 0x4 is set)
            recs.append(fixmate_inputs.rec("n%d" % rs.randint(0, n_names), tid, pos, "%dM" % rs.randint(1, 40), flag))
        tl = [1000000] * 3
        cls = fixmate_ref.classes(recs, tl)
        names = [fixmate_ref.qname(r) for r in recs]
        for remove in (False, True):
            out, counts = fixmate_ref.machine(recs, tl, remove)
            roles, order = fixmate_ref.closed_form(cls, names, remove)
            assert order == [i for i, _ in out], (trial, remove)
            assert roles.count(fixmate_ref.FIRST) == roles.count(fixmate_ref.SECOND) == counts["pairs"], trial
            assert roles.count(fixmate_ref.SINGLE) == counts["singletons"] and roles.count(fixmate_ref.PENDING) <= 1, trial
            # a first's partner is the next live record, and the loop paired exactly those
            live = [i for i in range(n) if cls[i] == fixmate_ref.LIVE]
            for l, i in enumerate(live):
                if roles[i] == fixmate_ref.FIRST:
                    j = live[l + 1]
                    assert roles[j] == fixmate_ref.SECOND and order.index(j) == order.index(i) + 1, trial
                    mt = struct.unpack_from("<ii", dict(out)[i], 24)
                    assert mt == struct.unpack_from("<ii", recs[j], 4), trial


def build_host(tmp, sanitize):
    exe = os.path.join(tmp, "fixmate_host_san" if sanitize else "fixmate_host")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixmate_host_main.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("fixmate_host_" + request.param)), request.param == "sanitized")


def test_host_route(host_program, inputs, tmp_path):
    """every recorded case through the stand-alone program; what the reference leaves undefined is refused with status 2"""
    for case in CASES:
        err = run_case(host_program, case, inputs, tmp_path / case["id"])
        if case["input"] in UNDEFINED and len(case["args"]) >= 2:
            assert "the reference's behaviour is undefined here" in err, case["id"]


def test_outside_the_domain_is_said(host_program, inputs, tmp_path):
    """an input that is no BAM file and a name without its end: status 2 and a reason, no output"""
    (tmp_path / "text.bam").write_bytes(b"not a BAM file\n")
    from bai_inputs import bgzf, header, refs
    r = bytearray(fixmate_inputs.rec("abcd", 0, 5, "", 0x1))
    r[36:41] = b"abcde"
    (tmp_path / "endless.bam").write_bytes(bgzf([header(refs(3)), bytes(r) + bytes(r)]))
    for name, word in (("text.bam", b"no BAM file"), ("endless.bam", b"a read name runs past its record")):
        p = subprocess.run([host_program, name, "out.bam"], cwd=tmp_path, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2 and word in p.stderr, (name, p.stderr)
        assert not (tmp_path / "out.bam").exists()
