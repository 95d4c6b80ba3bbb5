"""CPU: the recorded runs of the reference's `samtools view` (tests/golden/view/manifest.json, made by
tests/golden/make_golden_view.py) against (a) the sequential restatement tests/view_ref.py -- main_samview's options, process_aln's
filters, drop_rg, samopen's text header, bam_format1_core, the writer's cuts -- and (b) the sequential route bin/bam_view falls
back to (highperformancengs_amd/csrc/host/bam_view_host.hpp) inside a stand-alone program with its own main
(tests/view_host_main.cpp), built plain and with g++ -fsanitize=address,undefined and run as a process of its own: nothing
sanitized is loaded into Python.  (c) The closed forms the device stands on -- the line's length from field widths, X31 as a
polynomial over 16 lanes, -s as a 24-bit integer threshold -- against the sequential forms on seeded random records.  The tool
on the device and the hpn_bam_view_* ABI: tests/test_view_gpu.py."""
import base64
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import view_inputs
import view_ref
from conftest import GOLDEN, PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLDEN, "view", "manifest.json")) as _f:
    MANIFEST = json.load(_f)
CASES = MANIFEST["cases"]
UNDEFINED = {"tid_beyond_header", "mtid_beyond_header"}
REFUSED = {"tid_beyond_header_text", "mtid_beyond_header_text", "region", "option_S", "option_t", "option_T", "option_L", "option_B"}
HOST_INPUTS = {"aux_float", "aux_a_nul", "name_nul_inside", "aux_unknown", "aux_b_negative"}


@pytest.fixture(scope="module")
def inputs():
    return view_inputs.inputs()


def check_blob(case, key, got):
    """`got`: the bytes, or None where there are none"""
    want = case[key]
    if want is None:
        assert got is None, (case["id"], key)
        return
    assert got is not None, (case["id"], key)
    assert len(got) == want["size"], (case["id"], key, len(got), want["size"])
    assert hashlib.sha256(got).hexdigest() == want["sha256"], (case["id"], key)
    if want["b64"] is not None:
        assert got == base64.b64decode(want["b64"]), (case["id"], key)


def run_case(exe, case, inputs, work, env=None, on_exit=None):
    """one recorded case through a program with view's arguments: stdout and the -o file byte for byte, stderr, status, what is left
    behind; where the reference's run was not recorded (`refuse`): status 2, a reason under [hpn], no output.  on_exit(status,
    stderr) is called before anything is checked.  -> stderr"""
    work.mkdir()
    data = inputs[case["input"]] if case["input"] else None
    given = [view_inputs.materialize(str(work), case["input"], data)] if case["input"] and not case["stdin"] else []
    for fn, text in case["files"].items():
        (work / fn).write_bytes(text.encode())
        given.append(fn)
    feed = {"input": data} if case["stdin"] else {"stdin": subprocess.DEVNULL}
    p = subprocess.run([exe] + case["args"], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env, **feed)
    err = p.stderr.decode("latin-1")
    if on_exit:
        on_exit(p.returncode, err)
    said = "".join(l + "\n" for l in err.splitlines() if not l.startswith("[hpn]"))
    left = sorted(fn for fn in os.listdir(work) if fn not in given)
    if case["expect"] == "refuse":
        assert p.returncode == 2 and "[hpn] bam_view:" in err and p.stdout == b"", (case["id"], p.returncode, err[-2000:])
        assert left == [], case["id"]
        return err
    assert p.returncode == case["rc"], (case["id"], p.returncode, err[-2000:])
    assert said == case["stderr"], (case["id"], said[-500:], case["stderr"][-500:])
    check_blob(case, "stdout", p.stdout)
    assert left == case["listing"], case["id"]
    check_blob(case, "file", (work / left[0]).read_bytes() if left else None)
    return err


def test_manifest_is_complete():
    ids = {c["id"] for c in CASES}
    for n in view_inputs.names():          # every input as text, as BAM and counted
        assert {n + "_text", n + "_b", n + "_c"} <= ids, n
    assert {"no_arguments", "long_help", "unknown_option", "missing_input", "truncated_mid_block_h", "truncated_mid_record_h", "no_eof_h", "mixed_stdin",
            "mixed_b_stdout", "mixed_pipe", "mixed_threads"} <= ids
    assert {c["id"] for c in CASES if c["expect"] == "refuse"} == REFUSED
    assert all(c["rc"] in (0, 1) and c["why"] is None for c in CASES if c["id"] not in REFUSED)
    assert MANIFEST["threads_change_nothing"] is True
    # the inputs the device hands to the host route, on text output; BAM output and the count of the same files stay on the device
    abandoned = {c["input"] for c in CASES if c["route"] == "abandoned" and c["rc"] == 0}
    assert abandoned == HOST_INPUTS | {"rg"}
    # the read-group rules run on the device; only -l over a header whose table the reference has words about goes to the host
    groups = [c for c in CASES if c["input"] in ("rg", "rg_clean") and any(a in c["args"] for a in ("-r", "-R", "-l"))]
    assert len(groups) >= 17 and {c["id"] for c in groups if c["route"] != "device"} == {"rg_l", "rg_l_b", "rg_r_l", "rg_l_c"}
    assert all("not unique" in c["stderr"] for c in groups if c["route"] != "device")
    assert {"rg_R_l", "rg_clean_R_l", "rg_clean_l", "rg_clean_r_l", "rg_r", "rg_R", "rg_R_b", "rg_R_h"} <= {c["id"] for c in groups if c["route"] == "device"}
    assert all(c["route"] == "device" for c in CASES if c["input"] in HOST_INPUTS and c["id"].endswith(("_b", "_c")) and "_s" not in c["id"])
    used = "".join(" ".join(c["args"]) + " " for c in CASES)
    for opt in ("-b", "-u", "-1", "-h", "-H", "-c", "-x", "-X", "-o", "-f", "-F", "-q", "-m", "-l", "-r", "-R", "-s", "-Q", "-@", "-?"):
        assert opt + " " in used, opt


def test_inputs_are_the_recorded_ones_and_hold_what_they_are_named_for(inputs):
    assert view_inputs.digests() == MANIFEST["inputs"]
    recs = lambda n: view_ref.parse(inputs[n]).recs
    cores = lambda n: [view_ref.core(r) for r in recs(n)]
    lens = {c["l_qseq"] for c in cores("lengths")}
    assert {0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257} <= lens
    assert {c["l_qname"] - 1 for c in cores("lengths")} >= {1, 15, 16, 17, 254}
    absent = [r for r in recs("lengths") if view_ref.core(r)["l_qseq"] and r[view_ref.layout(r)[2]] == 0xff]
    assert len(absent) >= 11
    codes = set()
    for r in recs("lengths"):
        _, sq, ql, _ = view_ref.layout(r)
        for b in r[sq:ql]:
            codes |= {b >> 4, b & 15}
    assert codes == set(range(16))
    nu = cores("numbers")
    assert {c["pos"] for c in nu} >= {-1, 0, 8, 9, 98, 99, (1 << 31) - 2} and {c["mpos"] for c in nu} >= {-1, (1 << 31) - 2}
    assert {c["isize"] for c in nu} >= {-(1 << 31), -1, 0, (1 << 31) - 1} and {c["mapq"] for c in nu} >= {0, 9, 10, 99, 100, 255}
    assert {c["flag"] for c in nu} >= {0, 0xffff} | {1 << b for b in range(16)} and {c["n_cigar"] for c in nu} >= {0, 1, 65535}
    ops = set()
    for r in recs("numbers"):
        c = view_ref.core(r)
        ops |= {(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % c["n_cigar"], r, 36 + c["l_qname"])}
    assert {op for op, _ in ops} == set(range(10)) and {ln for _, ln in ops} >= {0, (1 << 28) - 1}
    targets = view_ref.parse(inputs["aux_all"]).targets
    text = b"\n".join(view_ref.format_line(r, targets, 0) for r in recs("aux_all"))
    for piece in (b"c0:i:-128", b"C1:i:255", b"s0:i:-32768", b"S1:i:65535", b"i0:i:-2147483648", b"I1:i:4294967295", b"XA:A:!", b"Z0:Z:\t", b"H1:H:1AE301",
                  b"Bc:B:c,-128,0,127", b"BI:B:I,0,4294967295", b"Be:B:c\t", b"BE:B:I"):
        assert piece in text, piece
    assert max(len(r) for r in recs("aux_all")) > 60000 and b":f:" not in text and b":d:" not in text
    ftext = b"\n".join(view_ref.format_line(r, targets, 0) for r in recs("aux_float"))
    for piece in (b"XF:f:1e+06", b"XF:f:123456", b"XF:f:1.23457e+06", b"XF:f:1e-05", b"XF:f:inf", b"XF:f:-inf", b"XF:f:nan", b"XD:d:2.5e-300", b"BF:B:f,0,1,-1.5"):
        assert piece in ftext, piece
    o = view_ref.options([])
    reason = lambda n: view_ref.device_reason(recs(n), 3, o)[1]
    assert [reason(n) for n in ("aux_float", "aux_a_nul", "name_nul_inside", "aux_unknown", "aux_b_negative", "tid_beyond_header", "mtid_beyond_header")] == [
        view_ref.R_FLOAT, view_ref.R_ANUL, view_ref.R_NAME, view_ref.R_AUXTYPE, view_ref.R_AUXTYPE, view_ref.R_TARGET, view_ref.R_TARGET]
    # rg: Z and another type, none, an unknown ID; the header's table
    rg = [view_ref.aux_rg(r) for r in recs("rg")]
    assert None in rg and {recs("rg")[i][at:at + 1] for i, at in enumerate(rg) if at} == {b"Z", b"C"}
    assert view_ref.rg_table(view_ref.parse(inputs["rg"]).text) == {b"a1": b"libB", b"a2": b"libA", b"b1": b"libB"}
    assert view_ref.rg_messages(view_ref.parse(inputs["rg"]).text) and not view_ref.rg_messages(view_ref.parse(inputs["rg_clean"]).text)
    assert view_ref.rg_table(view_ref.parse(inputs["rg_clean"]).text) == {b"a1": b"libA", b"a2": b"libA", b"b1": b"libB"}
    # subsample: pairs share a name, signed bytes, one-byte names
    names = [r[36:36 + view_ref.core(r)["l_qname"] - 1] for r in recs("subsample")]
    assert names[0] == names[1] and any(max(n) >= 0x80 for n in names) and sum(1 for n in names if len(n) == 1) == 5
    # runs: kept and dropped runs of 2,047, 2,048 and 2,049
    flags = [c["flag"] & 0x400 for c in cores("runs")]
    runs, at = [], 0
    while at < len(flags):
        e = at
        while e < len(flags) and flags[e] == flags[at]:
            e += 1
        runs.append((flags[at], e - at))
        at = e
    T = view_inputs.SCAN_TILE
    assert runs == [(0, T - 1), (0x400, T - 1), (0, T), (0x400, T), (0, T + 1), (0x400, T + 1)]
    lo = cores("last_only")
    assert all(c["flag"] & 0x400 for c in lo[:-1]) and not lo[-1]["flag"] & 0x400 and len(lo) > T and recs("no_records") == []
    # cuts: the kept records in front of the long one fill a block exactly, by one less, by one more
    for n, d in (("cuts_exact", 0), ("cuts_less", -1), ("cuts_more", 1)):
        kept = [r for r in recs(n) if not view_ref.core(r)["flag"] & 0x400]
        k = next(i for i, r in enumerate(kept) if len(r) > view_inputs.FULL)
        assert sum(len(r) for r in kept[:k]) == view_inputs.FULL + d, n
        # -Q 2: the long record starts a block of its own (it never fits behind another), the writer cuts it FULL bytes in, and that
        # cut lies inside its quality bytes, every one of which the scale changes
        _, _, ql, ax = view_ref.layout(kept[k])
        assert ql < view_inputs.FULL < ax and all(view_ref.scaled(kept[k], 2)[j] != kept[k][j] for j in (ql, view_inputs.FULL - 1, view_inputs.FULL, ax - 1)), n
        blocks = view_ref.cut(b"", [view_ref.scaled(r, 2) for r in kept])
        first = next(j for j, blk in enumerate(blocks) if blk[:len(kept[k])][36:40] == b"long")
        assert len(blocks[first]) == view_inputs.FULL and blocks[first][ql:] + blocks[first + 1][:ax - view_inputs.FULL] == view_ref.scaled(kept[k], 2)[ql:ax], n
    assert len(recs("mixed")) == 3000


def test_restatement(inputs):
    """the restatement against every recorded run the reference finished"""
    for case in CASES:
        data = inputs[case["input"]] if case["input"] else None
        files = {k: v.encode() for k, v in case["files"].items()}
        out, made, err, rc = view_ref.view(data, case["args"], files, case["stdin"])
        if case["expect"] == "refuse":
            assert rc == 2, case["id"]
            continue
        assert rc == case["rc"] and err == case["stderr"], case["id"]
        check_blob(case, "stdout", out)
        check_blob(case, "file", made)


def test_routes(inputs):
    for case in CASES:
        if case["expect"] == "same" and case["input"]:
            files = {k: v.encode() for k, v in case["files"].items()}
            assert case["route"] == view_ref.route(inputs[case["input"]], case["args"], case["stdin"], files), case["id"]


def test_this_machines_rand_is_the_recorded_one():
    """-s with a non-zero seed calls the C library's srand and rand: the recorded runs hold only where they give what they gave"""
    for seed, want in MANIFEST["rand"].items():
        got = view_ref.libc_rand(int(seed))
        assert got == want, "srand(%s); rand() gives %d on this machine, the manifest recorded %d: the -s cases with a seed cannot hold" % (seed, got, want)


def random_records(rs, n):
    out = []
    for k in range(n):
        aux = b""
        for _ in range(int(rs.randint(0, 6))):
            kind = rs.randint(0, 10)
            key = bytes(rs.randint(65, 91, 2).tolist())
            if kind < 6:
                t = "cCsSiI"[kind]
                lo, hi = {"c": (-128, 128), "C": (0, 256), "s": (-32768, 32768), "S": (0, 65536), "i": (-(1 << 31), 1 << 31), "I": (0, 1 << 32)}[t]
                v = int(rs.choice([lo, hi - 1, 0, 9, 10, -1 if lo < 0 else 99, int(rs.randint(lo, hi, dtype=np.int64))]))
                aux += view_inputs.aux_i(key, t, v)
            elif kind == 6:
                aux += key + b"A" + bytes([int(rs.randint(33, 127))])
            elif kind == 7:
                aux += key + b"ZH"[rs.randint(0, 2):][:1] + bytes(rs.randint(33, 127, int(rs.randint(0, 40))).tolist()) + b"\0"
            else:
                t = "cCsSiI"[rs.randint(0, 6)]
                lo, hi = {"c": (-128, 128), "C": (0, 256), "s": (-32768, 32768), "S": (0, 65536), "i": (-(1 << 31), 1 << 31), "I": (0, 1 << 32)}[t]
                aux += view_inputs.aux_b(key, t, [int(v) for v in rs.randint(lo, hi, int(rs.randint(0, 9)), dtype=np.int64)])
        n_seq = int(rs.choice([0, 1, 2, 15, 16, 17, 33, int(rs.randint(0, 200))]))
        edge = lambda: int(rs.choice([-1, 0, 8, 9, 98, 99, 999999998, 999999999, (1 << 31) - 2, int(rs.randint(0, 1 << 30))]))
        name = bytes(rs.randint(1, 256, int(rs.randint(1, 40))).tolist()).replace(b"\0", b"x")
        cg = [(int(rs.choice([0, 9, 10, (1 << 28) - 1, int(rs.randint(0, 1000))])), int(rs.randint(0, 10))) for _ in range(int(rs.randint(0, 6)))]
        out.append(view_inputs.rec(name, int(rs.randint(-1, 3)), edge(), cg, int(rs.randint(0, 1 << 16)), int(rs.randint(0, 256)), rs.randint(0, 16, n_seq).tolist(),
                                   None if rs.randint(0, 4) == 0 else rs.randint(0, 94, n_seq).tolist(), int(rs.randint(-1, 3)), edge(),
                                   int(rs.choice([-(1 << 31), (1 << 31) - 1, 0, -1, int(rs.randint(-5000, 5000))])), aux))
    return out


def test_closed_forms_are_the_sequential_ones():
    """on 3,000 seeded random records with every integer aux type: the line's length against len(format(record)) in the three flag
    styles and under -Q; X31 as a polynomial against the loop, signed bytes included"""
    rs = np.random.RandomState(20261021)
    targets = [(b"c0", 5), (b"chromosome_one", 7), (b"x", 9)]
    for r in random_records(rs, 3000):
        for style in (0, 1, 2):
            assert view_ref.line_length(r, targets, style) == len(view_ref.format_line(r, targets, style)) + 1
        assert view_ref.line_length(r, targets, 0, 2) == len(view_ref.format_line(view_ref.scaled(r, 2), targets, 0)) + 1
        name = r[36:36 + view_ref.core(r)["l_qname"] - 1]
        assert view_ref.x31_poly(name) == view_ref.x31(name)
    for name in (b"", b"a", b"\xff", b"\x80" * 17, bytes(range(1, 255))):
        assert view_ref.x31_poly(name) == view_ref.x31(name)


def test_the_integer_threshold_is_the_double_comparison():
    """every 24-bit value at a handful of fractions, among them fractions that are not multiples of 2^-24"""
    k = np.arange(1 << 24, dtype=np.uint32)
    as_double = k.astype(np.float64) / float(0x1000000)
    for frac in (0.5, 0.000001, 1.0, 0.9999999, 0.25, 1.0 / 3, 0.1, 2.0 ** -24, 2.0 ** -25, 1 - 2.0 ** -24, 1 - 2.0 ** -30, 5e-324, 123.0, 0.3333333):
        t = view_ref.threshold(frac)
        assert 0 <= t <= 1 << 24
        assert np.array_equal(as_double >= frac, k >= t), frac


def build_host(tmp, sanitize):
    exe = os.path.join(tmp, "view_host_san" if sanitize else "view_host")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "view_host_main.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("view_host_" + request.param)), request.param == "sanitized")


def test_host_route(host_program, inputs, tmp_path):
    """every recorded case through the stand-alone program; what the reference leaves undefined is refused with status 2"""
    for case in CASES:
        err = run_case(host_program, case, inputs, tmp_path / case["id"])
        if case["input"] in UNDEFINED and case["expect"] == "refuse":
            assert "the reference's behaviour is undefined here" in err, case["id"]


def test_outside_the_domain_is_said(host_program, inputs, tmp_path):
    """an input that is no BAM file, a record without a name and an aux field past its record: status 2 and a reason, no output"""
    (tmp_path / "text.bam").write_bytes(b"not a BAM file\n")
    from bai_inputs import bgzf, header, refs
    r = bytearray(view_inputs.rec("abcd", 0, 5, "", 0x1))
    r[12] = 0
    (tmp_path / "noname.bam").write_bytes(bgzf([header(refs(3)), bytes(r)]))
    (tmp_path / "auxpast.bam").write_bytes(bgzf([header(refs(3)), view_inputs.rec("abcd", 0, 5, aux=b"NMi\x01\x02")]))
    for name, word in (("text.bam", b"no BAM file"), ("noname.bam", b"l_qname 0"), ("auxpast.bam", b"an aux field runs past its record")):
        p = subprocess.run([host_program, "-o", "out.sam", name], cwd=tmp_path, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2 and word in p.stderr and p.stdout == b"", (name, p.stderr)
        assert not (tmp_path / "out.sam").exists()
