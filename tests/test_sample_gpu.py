"""GPU: hpn_fastq_text_sample and bin/gzfastq_sample against the reference's recorded outputs (tests/golden/sample/)
and, on random text, against the Python restatement that test_sample_golden.py pins to them."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sample_ref
from test_sample_golden import CASES, GOLDEN, check_outputs, read_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def random_fastq(seed, n, final_newline=True, max_name=1022):
    """Names of 1 .. max_name bytes (with '@', any byte but '\\n' and NUL, bytes >= 0x80 included), reads of 0 .. 500 bases."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ln = int(rs.choice([1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 271, 272, 273, 1021, 1022])) if rs.rand() < 0.3 else int(rs.randint(1, max_name + 1))
        ln = min(ln, max_name)
        name = rs.randint(1, 256, ln).astype(np.uint8)
        name[name == 10] = 32
        name[0] = ord("@")
        rl = 0 if rs.rand() < 0.05 else int(rs.randint(0, 501))
        seq = rs.choice(np.frombuffer(b"ACGTN", np.uint8), rl).tobytes()
        ql = rl if rs.rand() < 0.9 else int(rs.randint(0, 501))      # a quality line of another length is regular here
        if i == n - 1:
            ql = max(ql, 1)      # (an empty last line without its newline is a stream that ends inside a record)
        qual = rs.randint(33, 127, ql).astype(np.uint8).tobytes()
        plus = b"+" if rs.rand() < 0.8 else (b"" if rs.rand() < 0.5 else b"+" + name[1:40].tobytes())
        out.append(name.tobytes() + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n")
    text = b"".join(out)
    return text if final_newline else text[:-1]


def run_stream(ctx, text, cuts, **rule):
    ctx.text_begin()
    got, kept, n_rec, n_kept, a = b"", [], 0, 0, 0
    for c in cuts:
        o, k, info = ctx.fastq_text_sample(text[a:c], last=(c == cuts[-1]), **rule)
        assert info.irregular == 0, info.irregular
        assert len(o) == info.n_bytes and len(k) == info.n_kept
        got += o
        kept += [int(x) for x in k]
        n_rec += info.n_records
        n_kept += info.n_kept
        a = c
    return got, kept, n_rec, n_kept


def cut_lists(seed, n):
    rs = np.random.RandomState(seed)
    few = sorted(set(int(x) for x in rs.randint(0, n + 1, 7)) | {n})
    ones = sorted(set(range(1, min(n, 700))) | set(int(x) for x in rs.randint(0, n + 1, 5)) | {n})   # 1-byte chunks, then a few large ones
    return [[n], few, ones]


@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("fasta", [False, True])
def test_abi_on_random_text(ctx, fasta, final_newline):
    text = random_fastq(20 + fasta + 2 * final_newline, 700, final_newline)
    recs = sample_ref.frame(text)
    assert len(recs) == 700
    picks = sorted(int(x) for x in np.random.RandomState(5).choice(700, 150, replace=False))
    rules = [({"threshold": sample_ref.threshold(0.37), "seed_add": 0x9e3779b9}, sample_ref.keep_fraction(recs, 0x9e3779b9, sample_ref.threshold(0.37))),
             ({"threshold": 1 << 24}, list(range(700))),
             ({"threshold": 0}, []),
             ({"picks": np.array(picks, np.uint64)}, picks),
             ({"picks": np.zeros(0, np.uint64)}, [])]
    for rule, want_kept in rules:
        want = sample_ref.render(recs, want_kept, fasta)
        for cuts in cut_lists(3, len(text)):
            got, kept, n_rec, n_kept = run_stream(ctx, text, cuts, fasta=fasta, **rule)
            assert (n_rec, n_kept) == (700, len(want_kept))
            assert kept == want_kept
            assert got == want
    assert 0 < len(rules[0][1]) < 700


def test_abi_ordinals_beyond_32_bits(ctx):
    text = random_fastq(31, 300, max_name=80)
    recs = sample_ref.frame(text)
    for base in (0xFFFFFFFF - 100, (1 << 40) + 7, 9_999_999_999_999_999_990, (1 << 64) - 301):   # digit counts change inside the stream
        local = [3, 99, 100, 101, 250, 299]
        got, kept, _, _ = run_stream(ctx, text, [len(text) // 2, len(text)], picks=np.array([base + i for i in local], np.uint64), first_ordinal=base)
        assert kept == [base + i for i in local]
        assert got == sample_ref.render(recs, local, first_ordinal=base)
        thr = sample_ref.threshold(0.5)
        got, kept, _, _ = run_stream(ctx, text, [len(text)], threshold=thr, first_ordinal=base, fasta=True)
        want = sample_ref.keep_fraction(recs, 0, thr)
        assert kept == [base + i for i in want] and got == sample_ref.render(recs, want, True, first_ordinal=base)


def test_abi_short_capacity_is_refused_and_nothing_is_overrun(ctx):
    from highperformancengs_amd import _lib
    text = np.frombuffer(random_fastq(41, 200, max_name=100), np.uint8)
    recs = sample_ref.frame(text.tobytes())
    need = len(sample_ref.render(recs, range(200)))
    rule = _lib.SampleRule(mode=_lib.SAMPLE_FRACTION, threshold=1 << 24)
    info = _lib.SampleInfo()
    out = np.full(need + 4096, 0xA5, np.uint8)
    kept = np.full(400, 0xA5A5A5A5A5A5A5A5, np.uint64)
    for out_cap, kept_cap, ok in ((need - 1, 400, False), (need, 199, False), (0, 400, False), (need, 200, True)):
        out[:] = 0xA5
        kept[:] = 0xA5A5A5A5A5A5A5A5
        ctx.text_begin()
        rc = ctx.L.hpn_fastq_text_sample(ctx.h, C.c_void_p(text.ctypes.data), text.size, 1, C.byref(rule), C.c_void_p(out.ctypes.data), out_cap,
                                         C.c_void_p(kept.ctypes.data), kept_cap, C.byref(info))
        if ok:
            assert rc == 0 and info.n_bytes == need and info.n_kept == 200
            assert out[:need].tobytes() == sample_ref.render(recs, range(200))
            assert (out[need:] == 0xA5).all() and (kept[200:] == 0xA5A5A5A5A5A5A5A5).all()
        else:
            assert rc == _lib.E_CAPACITY, (rc, out_cap, kept_cap)
            assert (out == 0xA5).all() and (kept == 0xA5A5A5A5A5A5A5A5).all()


def test_abi_reports_irregular_text_and_takes_ragged_quality(ctx):
    from highperformancengs_amd import _lib
    thr = 1 << 24
    for rel, flag in (("fastq/trunc.fq", _lib.TEXT_PARTIAL), ("fastq/longname.fq", _lib.TEXT_LONG_LINE)):
        ctx.text_begin()
        o, k, info = ctx.fastq_text_sample(read_input(rel), last=True, threshold=thr)
        assert info.irregular & flag and o == b"" and len(k) == 0
    ctx.text_begin()
    o, k, info = ctx.fastq_text_sample(b"@a\nAC\0T\n+\nIIII\n", last=True, threshold=thr)
    assert info.irregular & _lib.TEXT_NUL
    for rel in ("fastq/stale.fq", "fastq/short.fq", "fastq/len0.fq", "fastq/allzero.fq", "fastq/nonl.fq", "fastq/crlf.fq"):
        text = read_input(rel)
        recs = sample_ref.frame(text)
        ctx.text_begin()
        o, k, info = ctx.fastq_text_sample(text, last=True, threshold=thr)
        assert info.irregular == 0 and o == sample_ref.render(recs, range(len(recs))) and info.n_records == len(recs)
    ctx.text_begin()
    o, k, info = ctx.fastq_text_sample(b"", last=True, threshold=thr)
    assert (info.irregular, info.n_records, info.n_kept, o) == (0, 0, 0, b"")


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, env=None, in1=None, in2=None):
    in1 = in1 or os.path.join(GOLDEN, case["in1"])
    in2 = in2 or (os.path.join(GOLDEN, case["in2"]) if case["in2"] else None)
    os.makedirs(cwd)
    p = subprocess.run([os.path.join(BIN, "gzfastq_sample"), "-1", in1] + (["-2", in2] if in2 else []) + case["args"], cwd=cwd,
                       env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    got = {}
    for fn in os.listdir(cwd):
        raw = open(os.path.join(cwd, fn), "rb").read()
        got[fn] = gzip.decompress(raw) if raw else None
    return p, got


def check_run(case, p, got, what):
    assert p.returncode == case["rc"], (what, p.stderr.decode())
    assert p.stdout == b""
    check_outputs(case, got)
    assert TIMES.sub("at T s", p.stderr.decode()) == case["stderr"], what


def bgzip(path_in, path_out, block):
    from highperformancengs_amd.bamio import _Bgzf
    text = read_input(path_in)
    with open(path_out, "wb") as fh:
        z = _Bgzf(fh)
        for i in range(0, len(text), block):
            z.write(text[i:i + block])
        z.close()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tool_matches_the_reference_on_every_route(case, tmp_path):
    is_gz = case["in1"].endswith(".gz")
    small = os.path.getsize(os.path.join(GOLDEN, case["in1"])) < 20000
    routes = [("default", {}), ("host framer", {"HPN_TEXT": "0"}),
              # the hooks build with forced small chunks: records straddle many chunk borders
              ("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099"})]
    if is_gz:
        routes += [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                   ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
                   ("host inflaters off", {"HPN_NO_MGZ": "1", "HPN_NO_PGZ": "1", "HPN_TEXT_CHUNK": "70001"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)
    # the inputs re-packed as bgzip under their own names: the BGZF blocks are inflated on the device
    packed = tmp_path / "packed"
    os.makedirs(packed)
    ins = []
    for rel in (case["in1"], case["in2"]):
        if rel:
            ins.append(str(packed / os.path.basename(rel)))
            bgzip(rel, ins[-1], 3000 if small else 40000)
        else:
            ins.append(None)
    for k, (what, env) in enumerate([("bgzip", {}), ("bgzip, sliced", {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"}), ("bgzip on the host", {"HPN_BAM_GPU": "0"})]):
        p, got = run_tool(case, tmp_path / ("b%d" % k), env, ins[0], ins[1])
        check_run(case, p, got, what)


@pytest.mark.parametrize("name", ["trunc.fq", "longname.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz"])
@pytest.mark.parametrize("args", [["-s", "3.999"], ["-n", "1"]])
def test_tool_refuses_what_the_reference_crashes_on(name, args, tmp_path):
    case = {"in1": "fastq/" + name, "in2": None, "args": args}
    for k, env in enumerate(({}, {"HPN_TEXT": "0"}, {"HPN_GZ_GPU": "1"})):
        p, _ = run_tool(case, tmp_path / ("r%d" % k), env)
        assert p.returncode == 2, (env, p.returncode, p.stderr.decode())
        assert b"gzfastq_sample: " in p.stderr and name.encode() in p.stderr


def test_tool_usage_errors(tmp_path):
    os.makedirs(tmp_path / "w")
    exe = os.path.join(BIN, "gzfastq_sample")
    p = subprocess.run([exe, "-s", "0.5"], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"-1" in p.stderr
    p = subprocess.run([exe, "-1", "no_such_file.fq", "-s", "0.5"], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"no_such_file.fq" in p.stderr and os.listdir(tmp_path / "w") == []
    # neither -s nor -n: nothing is written
    p = subprocess.run([exe, "-1", os.path.join(GOLDEN, "fastq", "t.fq")], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and os.listdir(tmp_path / "w") == []


def test_tool_on_a_larger_gzip_with_many_chunks(tmp_path):
    """~40 MB of text (several chunks and slices on every route), fraction and picks, both mates."""
    text1 = random_fastq(77, 3000, max_name=120) * 40
    text2 = random_fastq(78, 3000, max_name=90) * 40
    (tmp_path / "a_1.fq.gz").write_bytes(gzip.compress(text1, 1))
    (tmp_path / "a_2.fq.gz").write_bytes(gzip.compress(text2, 1))
    args = ["-s", "5.2", "-n", "30000"]
    want, want_err = sample_ref.simulate(args, "a_1.fq.gz", text1, "a_2.fq.gz", text2)
    case = {"in1": None, "in2": None, "args": args}
    for k, env in enumerate(({}, {"HPN_GZ_GPU": "1"}, {"HPN_TEXT": "0"})):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env, str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz"))
        assert p.returncode == 0, p.stderr.decode()
        assert got == want and TIMES.sub("at T s", p.stderr.decode()) == want_err
