"""GPU: hpn_mrle_* and bin/gzfastq_mrle against the reference's recorded runs (tests/golden/mrle/) and, on random inputs, against
the Python restatement that test_mrle_golden.py pins to them: the packed file, the decoded text (made on the device from the
ENCODED bytes) and what one descriptor receives when both share it."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import mrle_inputs
import mrle_ref
from highperformancengs_amd import _lib
from test_mrle_golden import BY_ID, CASES, OWN, SAME, check_outputs, expected, input_path, read_input
from test_uniq_gpu import cut_lists

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")
INPUTS = mrle_inputs.own_inputs()
IN_DOMAIN = sorted(n for n in INPUTS if not n.startswith("bad_"))


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ------------------------------------------------------------------------------------------------------

def run_mrle(ctx, data, cuts=None, slice_bytes=1 << 24):
    ctx.mrle_begin()
    a, n = 0, 0
    cuts = cuts or [len(data)]
    for c in cuts:
        info = ctx.mrle_add(data[a:c], last=(c == cuts[-1]))
        assert info.irregular == 0, info.irregular
        n += info.n_records
        a = c
    res = ctx.mrle_finish()
    assert res.n_records == n and res.bad_record == -1
    outs = tuple(ctx.mrle_output(which, slice_bytes) for which in (_lib.MRLE_PACKED, _lib.MRLE_TEXT, _lib.MRLE_SHARED))
    assert [len(o) for o in outs] == list(res.out_bytes)
    return outs, res


def check_mrle(ctx, data, **kw):
    outs, res = run_mrle(ctx, data, **kw)
    want, _, n = mrle_ref.mrle(data)
    assert res.n_records == n
    for name, got, exp in zip(("packed", "text", "shared"), outs, want):
        assert got == exp, name
    assert outs[1] == b"".join(r[2] + b"\n" for r in mrle_ref.records(data))      # the device's decode gives the quality lines back
    return n


@pytest.mark.parametrize("name", IN_DOMAIN)
def test_every_constructed_input(ctx, name):
    """Line lengths 0 .. 1022, one-symbol runs of 1 .. 1022, runs across a lane's 16 bytes and a team's 256, savings of -1 / 0 / +1
    for each symbol, all flags and none, encoded sizes of 255 / 256 / 257 / 601, offsets of every alignment, empty inputs, text
    streams of 4,095 / 4,096 / 4,097 / 8,192 bytes, calls that end on a block edge, a packed stream of exactly 4,096 (mrle_inputs.py)
    -- whole, and cut into chunks."""
    text = INPUTS[name]
    lists = cut_lists(3, len(text), text) if len(text) < 6000 else [[len(text)], [len(text) // 3, len(text)]]
    for cuts in lists:
        check_mrle(ctx, text, cuts=cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 1000)


def test_the_worked_examples(ctx):
    (packed, text, shared), _ = run_mrle(ctx, INPUTS["examples.fq"])
    want = ["20 46 07", "00 46 46 23 23 46 46", "38 46 02 2f 37 37 3c 02 42 03", "20 46 fe", "20 46 ff 00", "20 46 ff ff 00", "01 23 ff ff 59"]
    assert packed == b"".join(bytes([len(bytes.fromhex(w))]) + bytes.fromhex(w) for w in want)
    assert shared == packed      # 1,656 bytes of text never leave their buffer
    (packed, _, _), _ = run_mrle(ctx, mrle_inputs.fq([b"F#" * 300, b""]))
    assert packed == b"\x59\x00" + b"F#" * 300 + b"\x01\x00"      # 601 encoded bytes behind the byte 0x59; an empty line is its flag byte


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 4097])
@pytest.mark.parametrize("mean_run", [1, 8, 60])
def test_random_lines(ctx, n, mean_run):
    """Lines of 0 .. 300 bytes (every 16th up to 1022) in runs of geometric length: one team, one wave and one more record, several
    workgroups, offsets of every alignment; whole and cut into two chunks inside a line."""
    rs = np.random.RandomState(1000 * mean_run + n)
    lengths = [int(rs.randint(0, 1023)) if k % 16 == 5 else int(rs.randint(0, 301)) for k in range(n)]
    text = mrle_inputs.fq(mrle_inputs.lines(7 * n + mean_run, lengths, mean_run))
    assert check_mrle(ctx, text) == n
    assert check_mrle(ctx, text, cuts=[len(text) // 2 + 1, len(text)], slice_bytes=5000) == n


def test_scan_crosses_tiles(ctx):
    from test_twobit_gpu import scan_tile
    n = 100_000
    assert n > 40 * scan_tile()      # uniq_scan_tiles: one tile per kScanTile sizes, a look-back hand-off between them
    rs = np.random.RandomState(5)
    text = mrle_inputs.fq(mrle_inputs.lines(6, rs.randint(0, 41, n)), seq=b"A")
    assert check_mrle(ctx, text, cuts=[len(text) // 3, len(text)], slice_bytes=1 << 20) == n


def test_out_of_domain_bytes(ctx):
    quals = mrle_inputs.lines(10, [37] * 40 + [0, 300, 1022])
    for bad in ([0], [42], [17], [30, 9, 22], [42, 0], [41]):
        q = list(quals)
        for k in bad:
            at = len(q[k]) - 1 if k % 2 else 0
            q[k] = q[k][:at] + (b"I" if k % 3 else b"\xff") + q[k][at + 1:]
        ctx.mrle_begin()
        ctx.mrle_add(mrle_inputs.fq(q), last=True)
        res = _lib.MrleResult()
        assert ctx.L.hpn_mrle_finish(ctx.h, C.byref(res)) == _lib.E_DOMAIN
        assert res.bad_record == min(bad) == mrle_ref.first_bad(q)
        assert b"record %d " % min(bad) in ctx.L.hpn_ctx_last_error(ctx.h)
        got = C.c_uint64(0)
        assert ctx.L.hpn_mrle_write(ctx.h, _lib.MRLE_PACKED, 0, None, 0, C.byref(got)) == _lib.E_STATE      # the session is closed
        assert check_mrle(ctx, mrle_inputs.fq(quals)) == 43      # a later session on the same context works
    # a byte outside the six in a name or a sequence is nobody's business
    assert check_mrle(ctx, b"@n\xe9 I\nACGTI\n+\nFF#F\n") == 1
    for name in ("bad_first.fq", "bad_mid.fq", "bad_last.fq"):
        ctx.mrle_begin()
        ctx.mrle_add(INPUTS[name], last=True)
        res = _lib.MrleResult()
        assert ctx.L.hpn_mrle_finish(ctx.h, C.byref(res)) == _lib.E_DOMAIN
        assert res.bad_record == {"bad_first.fq": 0, "bad_mid.fq": 5, "bad_last.fq": 11}[name]


def test_capacity_state_and_irregular_text(ctx):
    text = INPUTS["reads150.fq"]
    info, res = _lib.SortInfo(), _lib.MrleResult()
    buf = np.frombuffer(text, np.uint8)
    for max_bytes, ok in ((len(text) - 1, False), (len(text), True)):
        ctx.mrle_begin(max_bytes=max_bytes)
        half = len(text) // 2
        assert ctx.L.hpn_mrle_add(ctx.h, C.c_void_p(buf.ctypes.data), half, 0, C.byref(info)) == 0
        rc = ctx.L.hpn_mrle_add(ctx.h, C.c_void_p(buf.ctypes.data + half), len(text) - half, 1, C.byref(info))
        if ok:
            assert rc == 0 and info.store_bytes == len(text)
            assert ctx.L.hpn_mrle_finish(ctx.h, C.byref(res)) == 0 and res.n_records == 500
        else:
            assert rc == _lib.E_CAPACITY and str(len(text)).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
            assert ctx.L.hpn_mrle_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    ctx.mrle_begin()
    ctx.mrle_add(text[:100])
    got = C.c_uint64(7)
    assert ctx.L.hpn_mrle_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    assert ctx.L.hpn_mrle_write(ctx.h, _lib.MRLE_TEXT, 0, None, 0, C.byref(got)) == _lib.E_STATE
    ctx.mrle_add(text[100:], last=True)
    assert ctx.L.hpn_mrle_add(ctx.h, C.c_void_p(buf.ctypes.data), 10, 0, C.byref(info)) == _lib.E_STATE
    res = ctx.mrle_finish()
    assert ctx.L.hpn_mrle_write(ctx.h, _lib.MRLE_PACKED, res.out_bytes[0] + 1, None, 0, C.byref(got)) == _lib.E_ARG
    assert ctx.L.hpn_mrle_write(ctx.h, 3, 0, None, 0, C.byref(got)) == _lib.E_ARG and got.value == 0
    assert ctx.L.hpn_mrle_write(ctx.h, -1, 0, None, 0, C.byref(got)) == _lib.E_ARG
    # sessions of other families on the same context are not disturbed, nor is this one by them
    ctx.sort_begin()
    ctx.sort_add(text, last=True)
    ctx.twobit_pack_begin()
    ctx.twobit_pack_add(text, last=True)
    assert ctx.mrle_output(_lib.MRLE_TEXT) == mrle_ref.mrle(text)[0][1]
    assert ctx.sort_finish().n_records == 500 and ctx.twobit_pack_finish().n_records == 500
    for bad, flag in ((read_input("fastq/trunc.fq"), _lib.TEXT_PARTIAL), (read_input("fastq/longname.fq"), _lib.TEXT_LONG_LINE),
                      (b"@a\nACGT\n+\nFF\0F\n", _lib.TEXT_NUL), (b"@a\nACGT\n+\nFFFF\n@b\n", _lib.TEXT_PARTIAL)):
        ctx.mrle_begin()
        assert ctx.mrle_add(bad, last=True).irregular & flag
        assert ctx.L.hpn_mrle_finish(ctx.h, C.byref(_lib.MrleResult())) == _lib.E_STATE


def test_every_recorded_input(ctx):
    """The three outputs of the ABI against what the reference wrote: the file cases give the packed file and the text, the cases
    with a '-' prefix the shared descriptor."""
    seen = 0
    for case in SAME:
        if case["in"] is None:
            continue
        data = read_input(case["in"])
        if b"\0" in data:      # (irregular to the ABI; the tool frames it on the host)
            continue
        (packed, text, shared), _ = run_mrle(ctx, data)
        if case["outputs"]:
            check_outputs(case, text, {case["outputs"][0]["name"]: packed})
        else:
            check_outputs(case, shared, {})
        seen += 1
    assert seen >= 80


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, env=None, path=None):
    """Runs a manifest case's command in `cwd`.  path: another file than the case's input."""
    os.makedirs(cwd)
    path = path or (input_path(case["in"]) if case["in"] else None)
    cmd = [os.path.join(BIN, "gzfastq_mrle")] + [path if a == "{in}" else a for a in case["args"]]
    kw = {"stdin": open(path, "rb") if case["stdin"] == "file" else subprocess.DEVNULL}
    p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    files = {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd)}
    files.pop("no_such_file.fq", None)      # (a missing input is created, as the reference creates it)
    return p, files


def check_run(case, p, got, what):
    if case["expect"] == "refuse":
        assert p.returncode == 2 and p.stderr.startswith(b"gzfastq_mrle: ") and p.stderr.count(b"\n") == 1, (what, p.returncode, p.stderr.decode("latin-1"))
        assert p.stdout == b"" and not any(got.values()), what
        if case["why"] == "out-of-domain byte":
            first = mrle_ref.first_bad([r[2] for r in mrle_ref.records(read_input(case["in"]))])
            assert b"in record %d " % first in p.stderr, (what, p.stderr)
        return
    if case["expect"] == "usage":
        assert p.returncode == 1 and b"Usage" in p.stderr and p.stdout == b"" and got == {}, what
        return
    assert p.returncode == 0, (what, p.stderr.decode("latin-1"))
    check_outputs(case, p.stdout, got)
    assert TIMES.sub("at T s", p.stderr.decode("latin-1")) == case["stderr"], what
    stdout, files, _ = expected(case)
    assert (p.stdout, got) == (stdout, files), what


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tool_matches_the_reference(case, tmp_path):
    p, got = run_tool(case, tmp_path / "r")
    check_run(case, p, got, "default")
    if case["in"] and case["expect"] != "usage" and case["id"][:2] in ("g_", "s_"):
        p, got = run_tool(case, tmp_path / "h", {"HPN_TEXT": "0"})      # framed on the host
        check_run(case, p, got, "host framer")


@pytest.mark.parametrize("cid", ["f_reads150", "s_reads150", "s_mixed_noruns", "f_bad_mid"])
def test_gzfastq_mrle_on_every_route(cid, tmp_path):
    """The routes test_sort_gpu.py sends gzfastq_sort through, with the same switches of the hooks build; the input as it is, as
    one gzip member and as bgzip."""
    case = BY_ID[cid]
    text = read_input(case["in"])
    small = len(text) < 20000
    routes = [("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099", "HPN_TEXT_SLICE": "100" if small else "5000"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)
    from highperformancengs_amd.bamio import _Bgzf
    gz_routes = [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                 ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
                 ("host inflaters off", {"HPN_NO_MGZ": "1", "HPN_NO_PGZ": "1", "HPN_TEXT_CHUNK": "70001"})]
    for kind in ("bgzip", "gzip"):
        packed = tmp_path / kind
        os.makedirs(packed)
        path = str(packed / (os.path.basename(case["in"]) + ".gz"))
        if kind == "bgzip":
            with open(path, "wb") as fh:
                z = _Bgzf(fh)
                block = 3000 if small else 40000
                for i in range(0, len(text), block):
                    z.write(text[i:i + block])
                z.close()
        else:
            open(path, "wb").write(gzip.compress(text, 6))
        envs = [("bgzip", {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"})] if kind == "bgzip" else gz_routes
        for k, (what, env) in enumerate(envs):
            p, got = run_tool(case, tmp_path / ("%s_run%d" % (kind, k)), env, path)
            check_run(case, p, got, what)


def test_10000_reads_through_the_tool(tmp_path):
    """150-symbol lines as a sequencer with binned qualities writes them -- long runs of F, a tail of lower bins: the packed file,
    the text and the shared descriptor (1.5 MB of text blocks between 0.3 MB of packed ones)."""
    rs = np.random.RandomState(41)
    text = mrle_inputs.fq([mrle_inputs.line(rs, 150, 25) for _ in range(10_000)], seq=b"ACGT" * 37 + b"AC")
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(text, 1))
    (packed, lines, shared), err, n = mrle_ref.mrle(text)
    case = {"in": None, "args": ["-i", "{in}", "-o", "o"], "stdin": None}
    p, got = run_tool(case, tmp_path / "p", path=str(tmp_path / "a.fq.gz"))
    assert p.returncode == 0, p.stderr.decode("latin-1")
    assert got == {"o_sort_by_seq.fq": packed} and p.stdout == lines and len(lines) == 151 * 10_000
    assert TIMES.sub("at T s", p.stderr.decode()) == err and n == 10_000
    p, got = run_tool(dict(case, args=["-i", "{in}"]), tmp_path / "s", path=str(tmp_path / "a.fq.gz"))
    assert p.returncode == 0 and got == {} and p.stdout == shared
