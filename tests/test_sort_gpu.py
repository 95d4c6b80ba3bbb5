"""GPU: hpn_fastq_sort_* and bin/gzfastq_sort against the reference's recorded outputs (tests/golden/sort/) and, on random
text, against the Python restatement that test_sort_golden.py pins to them -- the output bytes, and the refinement's
bookkeeping (`rounds`, `refined`), which must EQUAL the restatement's."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import sort_ref
from test_sort_golden import CASES, GOLDEN, check_outputs, expected, input_path, read_input
from test_uniq_gpu import cut_lists, random_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def run_abi(ctx, data, by_name, cuts=None, slice_bytes=1 << 24):
    ctx.sort_begin(by_name=by_name)
    a, n = 0, 0
    cuts = cuts or [len(data)]
    for c in cuts:
        info = ctx.sort_add(data[a:c], last=(c == cuts[-1]))
        assert info.irregular == 0, info.irregular
        n += info.n_records
        a = c
    res = ctx.sort_finish()
    assert res.n_records == n
    out = ctx.sort_output(slice_bytes)
    assert len(out) == res.out_bytes
    return out, res


def check_against_ref(out, res, data, by_name, bookkeeping=True):
    want, _, r = sort_ref.simulate(data, by_name, r=1 << 40, bookkeeping=bookkeeping)
    assert res.n_records == r.n
    assert out == want
    if bookkeeping:
        assert (res.rounds, res.refined) == (r.rounds, r.refined), (r.tied, res.rounds, res.refined)
    return r


@pytest.mark.parametrize("by_name", [False, True])
@pytest.mark.parametrize("final_newline", [True, False])
def test_abi_on_random_text(ctx, final_newline, by_name):
    """uniq's random text: sequences of 0 .. 300 bytes with high bytes, drawn from a pool (ties), names of 1 .. 300 random bytes,
    short and long quality lines; cut into one-byte chunks, inside every line, and fetched in slices of 1,000 bytes."""
    text = random_reads(150 + final_newline, 900, 200, final_newline)
    for cuts in cut_lists(3, len(text), text):
        out, res = run_abi(ctx, text, by_name, cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 1000)
        r = check_against_ref(out, res, text, by_name)
    assert r.n == 900
    # Random names and pooled sequences seldom agree in length AND in their first 6 bytes without being equal, so that text may
    # be settled by round 0 alone.  The same reads under names that differ only behind a 22-byte prefix (high bytes in it) cannot
    # be: 900 distinct names of 25 bytes agree in their first 6 and 14 bytes, so rounds 1 and 2 both have work.
    prefixed = random_reads(150 + final_newline, 900, 200, final_newline, names=lambda rs, i: b"@pr\xe9fix\xff:shared:by:all%03d" % i)
    for cuts in cut_lists(3, len(prefixed), prefixed):
        out, res = run_abi(ctx, prefixed, by_name, cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 1000)
        r = check_against_ref(out, res, prefixed, by_name)
    assert r.n == 900 and (r.rounds >= 3 if by_name else r.rounds >= 1)


def test_abi_duplicate_names_and_prefixes(ctx):
    names = lambda rs, i: [b"@dup", b"@dup 1", b"@A00123:456:HXXXXXXXX:1:1101:%d:%d 1:N:0:ACGT" % (int(rs.randint(1000, 1040)), int(rs.randint(1000, 1040)))][int(rs.randint(0, 3))]
    text = random_reads(160, 3000, 100, max_len=80, names=names)
    for by_name in (True, False):
        out, res = run_abi(ctx, text, by_name)
        r = check_against_ref(out, res, text, by_name)
    assert r.n == 3000


def test_abi_every_golden_input(ctx):
    seen = set()
    for case in CASES:
        if case["expect"] != "same" or case["rc"] or case["in"] is None or case["stdin"] == "pipe" or (case["in"], case["by_name"]) in seen:
            continue
        data = read_input(case["in"])
        if b"\0" in data:      # (irregular to the ABI; the tool frames it on the host)
            continue
        seen.add((case["in"], case["by_name"]))
        out, res = run_abi(ctx, data, case["by_name"])
        check_against_ref(out, res, data, case["by_name"])
        stdout, files, _, _ = expected(case)
        assert out == (stdout or next(iter(files.values()), b""))
    assert len(seen) >= 40


def test_abi_edges_all_identical_and_empty(ctx):
    same = b"".join(b"@s%d\nACGTACGTACGTACGTACGTAC\n+\n%s\n" % (i % 50, bytes([33 + (i * 7) % 60]) * 22) for i in range(20000))
    out, res = run_abi(ctx, same, False)
    r = check_against_ref(out, res, same, False)
    assert (r.rounds, r.refined) == (1, 0)      # duplicates leave after one look
    out, res = run_abi(ctx, same, True)
    check_against_ref(out, res, same, True)
    out, res = run_abi(ctx, b"", False)
    assert (res.n_records, res.rounds, res.refined, res.out_bytes, out) == (0, 0, 0, 0, b"")
    one = b"@only\nACGT\n+\nIIII\n"
    out, res = run_abi(ctx, one, True)
    assert (out, res.rounds, res.refined) == (one, 1, 0)
    # more than one line per four bytes is regular here, and so is a quality line shorter than its sequence
    dense = b"@\n\n+\n\n" * 5000 + b"@\nA\n+\n!\n" * 3 + b"@b\nACGTAC\n+\nII\n"
    out, res = run_abi(ctx, dense, False)
    check_against_ref(out, res, dense, False)


def million(seed, n, n_keys, length, name):
    rs = np.random.RandomState(seed)
    pool = rs.choice(ACGT, (n_keys, length))
    pick = np.concatenate([np.arange(n_keys), rs.randint(0, n_keys, n - n_keys)])
    rs.shuffle(pick)
    seqs = [bytes(x) for x in pool[pick]]
    qual = bytes(rs.randint(33, 74, length).astype(np.uint8))
    return b"".join(b"%s\n%s\n+\n%s\n" % (name(rs, i), seqs[i], qual) for i in range(n))


def test_bookkeeping_on_a_million_distinct_reads(ctx):
    """1e6 uniform random 150 bp reads: all of them are still tied after 6 bytes (4^6 prefixes), about 4^-14 N^2 / 2 = 1,900
    pairs after 14, practically none after 22 -- refined is N and a few thousand, against the 19 N of a walk over all words."""
    n = 1_000_000
    text = million(31, n, n, 150, lambda rs, i: b"@r%d" % i)
    cuts = list(range(8 << 20, len(text), 8 << 20)) + [len(text)]
    out, res = run_abi(ctx, text, False, cuts, slice_bytes=4 << 20)
    r = check_against_ref(out, res, text, False)
    assert r.n == n and n < r.refined < n + 10_000 and r.rounds in (3, 4)


def test_bookkeeping_on_reads_with_duplicates(ctx):
    n, n_keys = 1_000_000, 700_000      # ~30 % of the reads repeat an earlier sequence
    text = million(32, n, n_keys, 50, lambda rs, i: b"@read%d" % i)
    cuts = list(range(8 << 20, len(text), 8 << 20)) + [len(text)]
    out, res = run_abi(ctx, text, False, cuts, slice_bytes=4 << 20)
    r = check_against_ref(out, res, text, False)
    assert r.n == n and r.refined < 2 * n


def test_bookkeeping_on_illumina_names(ctx):
    name = lambda rs, i: b"@A00123:456:HXXXXXXXX:%d:%d:%d:%d %d:N:0:ACGTACGT" % (1 + i % 4, 1101 + int(rs.randint(0, 78)), int(rs.randint(1000, 33000)),
                                                                                   int(rs.randint(1000, 33000)), 1 + i % 2)
    n = 300_000
    text = million(33, n, n, 36, name)
    out, res = run_abi(ctx, text, True, slice_bytes=4 << 20)
    r = check_against_ref(out, res, text, True)
    assert r.n == n and r.rounds >= 5      # the flow cell and lane are 22 bytes that decide nothing


def test_abi_capacity_and_state(ctx):
    from highperformancengs_amd import _lib
    text = random_reads(81, 200, 50, max_len=80)
    info, res = _lib.SortInfo(), _lib.SortResult()
    buf = np.frombuffer(text, np.uint8)
    for max_bytes, ok in ((len(text) - 1, False), (len(text), True)):
        ctx.sort_begin(max_bytes=max_bytes)
        half = len(text) // 2
        assert ctx.L.hpn_fastq_sort_add(ctx.h, C.c_void_p(buf.ctypes.data), half, 0, C.byref(info)) == 0
        rc = ctx.L.hpn_fastq_sort_add(ctx.h, C.c_void_p(buf.ctypes.data + half), len(text) - half, 1, C.byref(info))
        if ok:
            assert rc == 0 and info.store_bytes == len(text)
            assert ctx.L.hpn_fastq_sort_finish(ctx.h, C.byref(res)) == 0 and res.n_records == 200
        else:
            assert rc == _lib.E_CAPACITY
            assert str(len(text)).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
            assert ctx.L.hpn_fastq_sort_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    # finish before the last chunk, output before finish, a chunk behind the last one
    ctx.sort_begin()
    ctx.sort_add(text[:100])
    got = C.c_uint64(0)
    assert ctx.L.hpn_fastq_sort_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    assert ctx.L.hpn_fastq_sort_write(ctx.h, 0, None, 0, C.byref(got)) == _lib.E_STATE
    ctx.sort_add(text[100:], last=True)
    assert ctx.L.hpn_fastq_sort_add(ctx.h, C.c_void_p(buf.ctypes.data), 10, 0, C.byref(info)) == _lib.E_STATE
    res = ctx.sort_finish()
    assert ctx.L.hpn_fastq_sort_write(ctx.h, res.out_bytes + 1, None, 0, C.byref(got)) == _lib.E_ARG
    # a uniq session and a sort session of one context do not disturb each other
    ctx.uniq_begin()
    ctx.uniq_add(text, last=True)
    assert ctx.sort_output() == sort_ref.simulate(text, False, r=1 << 40)[0]
    assert ctx.uniq_finish().n_records == 200


def test_abi_reports_irregular_text(ctx):
    from highperformancengs_amd import _lib
    for text, flag in ((read_input("fastq/trunc.fq"), _lib.TEXT_PARTIAL), (read_input("fastq/longname.fq"), _lib.TEXT_LONG_LINE),
                       (b"@a\nAC\0T\n+\nIIII\n", _lib.TEXT_NUL), (b"@a\nACGT\n+\nIIII\n@b\n", _lib.TEXT_PARTIAL),
                       (read_input("sort/inputs/cut_plus.fq"), _lib.TEXT_PARTIAL)):
        ctx.sort_begin()
        info = ctx.sort_add(text, last=True)
        assert info.irregular & flag, (text[:20], info.irregular)
        assert ctx.L.hpn_fastq_sort_finish(ctx.h, C.byref(_lib.SortResult())) == _lib.E_STATE
    # a short quality line is harmless here
    ctx.sort_begin()
    assert ctx.sort_add(read_input("sort/inputs/shortq.fq"), last=True).irregular == 0
    assert ctx.sort_finish().n_records == 3


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, env=None, path=None):
    os.makedirs(cwd)
    path = path or (input_path(case["in"]) if case["in"] else None)
    cmd = [os.path.join(BIN, "gzfastq_sort")] + [path if a == "{in}" else a for a in case["args"]]
    kw = {"stdin": subprocess.DEVNULL}
    if case["stdin"] == "file":
        kw = {"stdin": open(path, "rb")}
    elif case["stdin"] == "pipe":
        kw = {"input": open(path, "rb").read()}
    p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    files = {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd)}
    files.pop("no_such_file.fq", None)      # (a missing input is created, as the reference creates it)
    return p, files


def check_run(case, p, got, what):
    if case["expect"] == "refuse":
        assert p.returncode == 2 and p.stderr.startswith(b"gzfastq_sort: ") and p.stderr.count(b"\n") == 1, (what, p.returncode, p.stderr.decode("latin-1"))
        assert p.stdout == b"" and not any(got.values()), what
        return
    if case["expect"] == "usage":
        assert p.returncode == 1 and b"Usage" in p.stderr and p.stdout == b"" and got == {}, what
        return
    assert p.returncode == case["rc"], (what, p.stderr.decode("latin-1"))
    check_outputs(case, p.stdout, got)
    assert TIMES.sub("at T s", p.stderr.decode("latin-1")) == case["stderr"], what
    if case["rc"] == 0:
        stdout, files, err, _ = expected(case)
        assert (p.stdout, got) == (stdout, files), what


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tool_matches_the_reference_on_every_route(case, tmp_path):
    if case["in"] is None or case["expect"] == "usage" or case["rc"] == 1:
        p, got = run_tool(case, tmp_path / "r")
        check_run(case, p, got, "default")
        return
    is_gz = case["in"].endswith(".gz")
    small = os.path.getsize(input_path(case["in"])) < 20000
    routes = [("default", {}), ("host framer", {"HPN_TEXT": "0"}),
              # the hooks build with forced small chunks and slices: records and output records straddle many borders
              ("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099", "HPN_TEXT_SLICE": "100" if small else "5000"})]
    if is_gz and case["stdin"] is None:
        routes += [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                   ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
                   ("host inflaters off", {"HPN_NO_MGZ": "1", "HPN_NO_PGZ": "1", "HPN_TEXT_CHUNK": "70001"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)
    if case["in"].startswith("fastq/bad") or case["stdin"] is not None:
        return      # (a damaged gzip stream cannot be re-packed)
    # the input re-packed as bgzip and as one gzip member under its own name
    from highperformancengs_amd.bamio import _Bgzf
    text = read_input(case["in"])
    for kind in ("bgzip", "gzip"):
        packed = tmp_path / kind
        os.makedirs(packed)
        path = str(packed / os.path.basename(case["in"]))
        if kind == "bgzip":
            with open(path, "wb") as fh:
                z = _Bgzf(fh)
                block = 3000 if small else 40000
                for i in range(0, len(text), block):
                    z.write(text[i:i + block])
                z.close()
        else:
            open(path, "wb").write(gzip.compress(text, 6))
        env = {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"} if kind == "bgzip" else {"HPN_GZ_GPU": "1"}
        p, got = run_tool(case, tmp_path / (kind + "_run"), env, path)
        check_run(case, p, got, kind)


def test_tool_on_a_larger_file_with_many_chunks(tmp_path):
    """~30 MB of text (several chunks and slices on every route), both modes, from a file, a gzip file and a pipe."""
    names = lambda rs, i: b"@SRR7.%d %d length=60" % (int(rs.randint(0, 3000)), i % 7)
    text = random_reads(191, 4000, 900, max_len=120, names=names) * 40
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(text, 1))
    (tmp_path / "a.fq").write_bytes(text)
    n = text.count(b"\n") // 4
    for by_name in (False, True):
        want, want_err, r = sort_ref.simulate(text, by_name, bookkeeping=False)
        name = "o_sort_by_name.fq" if by_name else "o_sort_by_seq.fq"
        mode = "-n" if by_name else "-s"
        runs = [({"in": None, "args": ["-i", "{in}", "-o", "o", mode], "stdin": None}, "a.fq.gz", {}, want_err),
                ({"in": None, "args": ["-i", "{in}", "-o", "o", mode], "stdin": None}, "a.fq.gz", {"HPN_GZ_GPU": "1"}, want_err),
                ({"in": None, "args": ["-i", "{in}", "-o", "o", mode], "stdin": None}, "a.fq", {"HPN_TEXT": "0"}, want_err),
                ({"in": None, "args": ["-o", "o", mode, "-r", str(n)], "stdin": "pipe"}, "a.fq.gz", {}, want_err[want_err.index("name:"):])]
        for k, (case, fn, env, err) in enumerate(runs):
            p, got = run_tool(case, tmp_path / ("r%d%d" % (k, by_name)), env, str(tmp_path / fn))
            assert p.returncode == 0, p.stderr.decode("latin-1")
            assert got == {name: want} and TIMES.sub("at T s", p.stderr.decode("latin-1")) == err, (k, by_name)
