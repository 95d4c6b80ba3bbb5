"""GPU: hpn_kseq_* and bin/map_kseq, bin/kbtree_kseq against the reference's recorded runs (tests/golden/kseq/manifest.json) and the
Python restatement that tests/test_kseq_golden.py pins to them.  Every case must take the route the classifier of
tests/kseq_ref.py gives its input -- the device's framing for "device", the host's parser for "host" -- case by case: a fallback
cannot hide a kernel that fails.  The shapes are the manifest's (tests/kseq_inputs.py): the refinement's seams, proper prefixes,
bytes >= 0x80, runs longer than a workgroup, every FASTA line layout and header form, one violation of each FASTQ condition,
record counts around the kernels' tiles; here they are also cut into chunks at every byte."""
import os
import re
import subprocess

import pytest

import kseq_inputs
import kseq_ref
from test_kseq_golden import CASES, check_blob, raw_input, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
SAME = [c for c in CASES if c["expect"] == "same"]
ROUTE = re.compile(rb"^\[hpn\] kseq: route (device|host)", re.M)


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def run_abi(ctx, data, cuts=None, slice_bytes=1 << 24):
    """(output, result) on the device's route, (None, irregular flags) where the device hands the text back"""
    from highperformancengs_amd import _lib
    ctx.kseq_begin()
    a, n = 0, 0
    cuts = cuts or [len(data)]
    for k, c in enumerate(cuts):
        info = ctx.kseq_add(data[a:c], last=(k == len(cuts) - 1))
        if info.irregular:
            assert info.irregular & (_lib.TEXT_KSEQ | _lib.TEXT_NUL) and info.n_records == 0
            return None, info.irregular
        n += info.n_records
        a = c
    res = ctx.kseq_finish()
    assert res.n_records == n
    out = ctx.kseq_output(slice_bytes)
    assert len(out) == res.out_bytes
    return out, res


def check_result(res, data):
    from highperformancengs_amd import _lib
    recs = kseq_ref.kseq_records(data)
    lens = kseq_ref.lengths(data)
    assert res.n_records == len(recs) and res.n_distinct == len({r.seq for r in recs})
    assert res.shape == ({0x3E: _lib.KSEQ_FASTA, 0x40: _lib.KSEQ_FASTQ}[data[0]] if data else _lib.KSEQ_NONE)
    assert res.one_length == (len(lens) <= 1)
    if lens:
        assert res.first_len == lens[0]
    if len(lens) > 1:
        assert res.other_len == lens[1]
    assert (res.rounds, res.refined) == kseq_ref.bookkeeping(data)


@pytest.mark.parametrize("case", [c for c in SAME if c["tool"] == "map_kseq" and c["stdin"] is None], ids=lambda c: c["id"])
def test_abi_every_recorded_case_takes_its_route(ctx, case):
    data = stream(case)
    out, res = run_abi(ctx, data)
    assert ("device" if out is not None else "host") == case["route"]
    if out is not None:
        check_blob(case["stdout"], out, case["id"])
        assert b"%d\n" % res.n_distinct == case["stderr"].encode("latin-1")
        check_result(res, data)


@pytest.mark.parametrize("name", ["cut_small.fa", "cut_small.fq"])
def test_abi_cut_at_every_byte(ctx, name):
    """two chunks, the cut at every offset: inside a header, between the lines of one wrapped sequence, behind a '\\r', inside the
    blocks that are passed over -- each cut's output equal to the uncut output"""
    data = kseq_inputs.own_inputs()[name]
    whole, res = run_abi(ctx, data)
    assert whole == kseq_ref.map_kseq(data)[0] and res.n_records == 5 and 3 <= res.n_distinct < 5      # (duplicates among them)
    for k in range(0, len(data) + 1):
        out, r = run_abi(ctx, data, [k, len(data)])
        assert out == whole, k
        assert (r.n_records, r.n_distinct) == (res.n_records, res.n_distinct), k


@pytest.mark.parametrize("name,piece", [("cut_small.fa", 1), ("cut_small.fq", 1), ("fa_w60.fa", 7), ("fa_crlf.fa", 3), ("fq_keys.fq", 5), ("fa_n257.fa", 64),
                                        ("fq_n257.fq", 61), ("fa_65535.fa", 4099)])
def test_abi_many_small_chunks(ctx, name, piece):
    """chunks of `piece` bytes (one byte: the unfinished record grows chunk by chunk), and an empty last chunk"""
    data = kseq_inputs.own_inputs()[name]
    whole, res = run_abi(ctx, data)
    assert whole == kseq_ref.map_kseq(data)[0]
    out, r = run_abi(ctx, data, list(range(piece, len(data), piece)) + [len(data), len(data)], slice_bytes=1000)
    assert out == whole and r.n_records == res.n_records


def test_abi_a_record_that_is_already_too_long_is_handed_back_early(ctx):
    """a joined sequence of 65,536 bytes in chunks of 4,099: the device says so while the record is still unfinished -- it does not
    hold the stream until the record's end arrives -- and the same chunks of the 65,535-byte file are framed"""
    from highperformancengs_amd import _lib
    data = kseq_inputs.own_inputs()["fa_65536.fa"]
    ctx.kseq_begin()
    for k, a in enumerate(range(0, len(data), 4099)):
        info = ctx.kseq_add(data[a:a + 4099], last=(a + 4099 >= len(data)))
        if info.irregular:
            break
    assert info.irregular == _lib.TEXT_KSEQ and 65536 < a + 4099 < 70000      # (the chunk that brings the 65,536th base, 70 to a line)
    data = kseq_inputs.own_inputs()["fa_65535.fa"]
    out, res = run_abi(ctx, data, list(range(4099, len(data), 4099)) + [len(data)])
    assert out == kseq_ref.map_kseq(data)[0] and res.n_records == 2


def test_abi_empty_stream_and_state(ctx):
    import highperformancengs_amd as hp
    out, res = run_abi(ctx, b"")
    assert out == b"" and (res.n_records, res.n_distinct, res.out_bytes, res.one_length) == (0, 0, 0, 1)
    ctx.kseq_begin()
    ctx.kseq_add(b">a\nAC\n")
    with pytest.raises(hp.HpnError):      # the stream has not had its last chunk
        ctx.kseq_finish()
    out, flags = run_abi(ctx, b"@a\nAC\n+\nII\n", [3, 11])      # a session after an abandoned one
    assert out == b"a (null)\nAC\n+\nII\n"
    ctx.kseq_begin()
    assert ctx.kseq_add(b"x>a\nAC\n", last=True).irregular      # text in front of the first header
    with pytest.raises(hp.HpnError):      # closed by the irregular chunk
        ctx.kseq_add(b">a\nAC\n", last=True)


def test_abi_the_earliest_of_equal_sequences_survives(ctx):
    """300 equal sequences (a run longer than a workgroup) under different names, comments and qualities, behind and in front of
    others: the first in input order is the one that is written"""
    data = kseq_inputs.own_inputs()["fq_run_300.fq"]
    out, res = run_abi(ctx, data)
    assert out == kseq_ref.map_kseq(data)[0]
    assert b"run0 c0\n" in out and b"run1 " not in out and res.n_records == 320 and res.n_distinct == 21


# ---- the tools ----------------------------------------------------------------------------------------------------

TOOL_IDS = ("g_", "b_", "stdin_", "missing_file", "no_arguments", "f_fq_keys", "f_fa_w", "f_fa_crlf", "f_fq_crlf", "f_fa_lone_cr", "f_fq_wrapped", "f_mixed",
            "f_nul", "f_fa_6553", "f_fq_headers", "f_fa_headers", "f_no_header", "f_text_in_front", "f_fa_passed_over", "f_fq_v_", "f_fa_cut",
            "f_fq_run_300", "f_fa_n2049", "f_fq_n2049", "f_fq_high_bytes", "f_fa_high_bytes", "f_fq_truncated", "f_fq_minus2", "f_fa_empty")


def run_tool(case, tmp_path, env_more=None):
    raw = raw_input(case)
    argv = [os.path.join(BIN, case["tool"])]
    if case["id"].startswith("no_arguments"):
        path = None
    elif raw is None:
        path = str(tmp_path / "no_such_file.fa")
        argv.append(path)
    else:
        path = str(tmp_path / os.path.basename(case["in"]))
        with open(path, "wb") as f:
            f.write(raw)
        argv.append(case["stdin"] if case["stdin"] is not None else path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update({"HPN_TIMING": "1"}, **(env_more or {}))
    p = subprocess.run(argv, cwd=tmp_path, stdin=open(path, "rb") if case["stdin"] is not None else subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=120)
    return p, path


@pytest.mark.parametrize("case", [c for c in CASES if c["id"].startswith(TOOL_IDS)], ids=lambda c: c["id"])
def test_tool_every_selected_case(case, tmp_path):
    p, path = run_tool(case, tmp_path)
    err = b"".join(l for l in p.stderr.splitlines(True) if not l.startswith(b"[hpn]"))
    if case["expect"] == "usage":
        assert p.returncode == 1 and p.stdout == b"" and b"Usage" in p.stderr
        return
    if case["expect"] == "refuse":
        assert p.returncode == 2 and p.stdout == b"", p.stderr
        assert {"damaged stream": b"damaged gzip stream", "NUL byte": b"NUL byte", "mixed lengths": b"sequences of "}[case["why"]] in p.stderr
        if case["why"] == "mixed lengths":
            a, b = kseq_ref.lengths(stream(case))[:2]
            assert b"sequences of %d and of %d bytes" % (a, b) in p.stderr
        return
    assert p.returncode == 0, p.stderr
    check_blob(case["stdout"], p.stdout, case["id"])
    assert err == case["stderr"].encode("latin-1")
    m = ROUTE.search(p.stderr)
    assert m and m.group(1).decode() == case["route"], p.stderr
    if case["id"] == "missing_file":
        assert os.path.getsize(path) == 0      # made, as the reference's O_CREAT makes it


@pytest.mark.parametrize("cid,chunk", [("f_fa_w60_fa", "64"), ("f_fq_keys_fq", "64"), ("f_fa_crlf_fa", "97"), ("f_fa_w60_fa_gz", "128"), ("stdin_dash_fq", "77"),
                                       ("b_fa_one_length_fa", "100")])
def test_tool_fed_in_small_chunks(cid, chunk, tmp_path):
    """the feed's chunks cut to a few dozen bytes (the hooks build's switch): the file, the gzip member and standard input"""
    case = next(c for c in CASES if c["id"] == cid)
    p, _ = run_tool(case, tmp_path, {"HPN_TEXT_CHUNK": chunk})
    assert p.returncode == 0, p.stderr
    check_blob(case["stdout"], p.stdout, cid)
    assert ROUTE.search(p.stderr).group(1) == b"device"


def test_tool_timing_lines_only_when_asked(tmp_path):
    case = next(c for c in CASES if c["id"] == "f_fq_keys_fq")
    p, _ = run_tool(case, tmp_path, {"HPN_TIMING": ""})
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    q = subprocess.run([os.path.join(BIN, "map_kseq"), str(tmp_path / "fq_keys.fq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert q.returncode == 0 and q.stderr == case["stderr"].encode("latin-1")
    check_blob(case["stdout"], q.stdout, "quiet")
