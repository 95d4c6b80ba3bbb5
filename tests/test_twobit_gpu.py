"""GPU: hpn_twobit_pack_*, hpn_twobit_unpack, bin/fastq2twobit and bin/twoBit2seq against the reference's recorded runs
(tests/golden/twobit/) and, on random inputs, against the Python restatement that test_twobit_golden.py pins to them."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import twobit_ref
from test_twobit_golden import BY_ID, CASES, SAME, case_input, check_outputs, expected, input_path, read_input
from test_uniq_gpu import cut_lists, random_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")
ACGTN = np.frombuffer(b"ACGTNacgtU", np.uint8)
LOW = bytes(b if b < 0x80 else (b & 0x7f if (b & 0x7f) not in (0, 10) else 65) for b in range(256))


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


def without_high_bytes(text):
    """The text with the bytes >= 0x80 of its SEQUENCE lines folded below (names and qualities keep theirs)."""
    lines = text.split(b"\n")
    for i in range(1, len(lines), 4):
        lines[i] = lines[i].translate(LOW)
    return b"\n".join(lines)


def fastq(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def random_seqs(seed, lengths):
    rs = np.random.RandomState(seed)
    return [bytes(rs.choice(ACGTN, int(n))) for n in lengths]


# ---- the ABI: pack ------------------------------------------------------------------------------------------------

def run_pack(ctx, data, cuts=None, slice_bytes=1 << 24):
    ctx.twobit_pack_begin()
    a, n = 0, 0
    cuts = cuts or [len(data)]
    for c in cuts:
        info = ctx.twobit_pack_add(data[a:c], last=(c == cuts[-1]))
        assert info.irregular == 0, info.irregular
        n += info.n_records
        a = c
    res = ctx.twobit_pack_finish()
    assert res.n_records == n and res.bad_record == -1
    out = ctx.twobit_pack_output(slice_bytes)
    assert len(out) == res.out_bytes
    return out, res


def check_pack(ctx, data, **kw):
    out, res = run_pack(ctx, data, **kw)
    want, _, n = twobit_ref.pack(data)
    assert res.n_records == n
    assert out == want
    assert (res.seq_len, res.packed_len) == ((want[0], want[1]) if want else (0, 0))
    return n


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097])
@pytest.mark.parametrize("final_newline", [True, False])
def test_pack_on_random_text(ctx, n, final_newline):
    """uniq's random text -- sequences of 0 .. 300 bytes of any kind, names with high bytes, short and long quality lines -- with
    the high bytes taken out of the sequences only; whole, cut into one-byte chunks and inside every line, fetched in slices of
    1,000 bytes."""
    text = without_high_bytes(random_reads(300 + n + final_newline, n, max(n // 2, 1), final_newline))
    lists = cut_lists(3, len(text), text)
    for cuts in (lists if n <= 257 else lists[:2]):
        assert check_pack(ctx, text, cuts=cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 1000) == n


def scan_tile():
    src = open(os.path.join(ROOT, "highperformancengs_amd", "csrc", "kernels", "radix_sort.hpp")).read()
    m = re.search(r"kScanTile = kScanThreads \* kScanItems;", src)
    assert m
    return int(re.search(r"kScanThreads = (\d+)", src).group(1)) * int(re.search(r"kScanItems = (\d+)", src).group(1))


def test_pack_scan_crosses_tiles(ctx):
    n = 100_000
    assert n > 40 * scan_tile()      # uniq_scan_tiles: one tile per kScanTile sizes, a look-back hand-off between them
    rs = np.random.RandomState(5)
    text = fastq(random_seqs(6, rs.randint(0, 41, n)))
    assert check_pack(ctx, text, cuts=[len(text) // 3, len(text)], slice_bytes=1 << 20) == n


def test_pack_every_length(ctx):
    seqs = random_seqs(7, range(71))
    for s in seqs:
        assert check_pack(ctx, fastq([s])) == 1
    assert check_pack(ctx, fastq(seqs)) == 71
    assert check_pack(ctx, fastq(seqs[::-1])) == 71
    for n in (255, 256, 257, 1021, 1022):      # the header is modulo 256; 1022: the longest line gzgets leaves whole
        assert check_pack(ctx, fastq(random_seqs(8, [3, n]))) == 2


def test_pack_edges(ctx):
    out, res = run_pack(ctx, b"")
    assert (out, res.n_records, res.out_bytes, res.seq_len, res.packed_len) == (b"", 0, 0, 0, 0)
    # the last record empty: header 00 00
    out, res = run_pack(ctx, fastq([b"ACGTACGTAC", b"GG", b""]))
    assert out == b"\x00\x00" + twobit_ref.pack_seq(b"GG") + twobit_ref.pack_seq(b"ACGTACGTAC")
    # only empty records: a header and nothing else
    assert run_pack(ctx, fastq([b"", b""]))[0] == b"\x00\x00"
    # every letter, both cases
    letters = bytes(range(1, 10)) + bytes(range(11, 128))
    assert check_pack(ctx, fastq([letters, letters[::-1]])) == 2
    # the last record's sequence with almost nothing behind it: "\n+\n" and one quality byte without its newline end the store
    for n in list(range(1, 41)) + [150]:
        s = random_seqs(9 + n, [n])[0]
        text = b"@x\nAC\n+\nII\n@last\n" + s + b"\n+\nI"
        assert check_pack(ctx, text) == 2


def test_pack_refuses_high_bytes(ctx):
    from highperformancengs_amd import _lib
    seqs = random_seqs(10, [37] * 40)
    for bad in ([0], [39], [17], [30, 9, 22], [39, 0]):
        s = list(seqs)
        for k in bad:
            s[k] = s[k][:36] + b"\x80" if k % 2 else b"\xff" + s[k][1:]
        ctx.twobit_pack_begin()
        ctx.twobit_pack_add(fastq(s), last=True)
        res = _lib.TwobitResult()
        assert ctx.L.hpn_twobit_pack_finish(ctx.h, C.byref(res)) == _lib.E_DOMAIN
        assert res.bad_record == min(bad) == twobit_ref.first_high(s)
        got = C.c_uint64(0)
        assert ctx.L.hpn_twobit_pack_write(ctx.h, 0, None, 0, C.byref(got)) == _lib.E_STATE      # the session is closed
        assert check_pack(ctx, fastq(seqs)) == 40      # a later session on the same context works
    # a high byte in a name or a quality line is nobody's business
    text = b"@n\xe9\nACGT\n+\n\xff\xfe\xfd\xfc\n"
    assert check_pack(ctx, text) == 1


def test_pack_capacity_state_and_irregular_text(ctx):
    from highperformancengs_amd import _lib
    text = fastq(random_seqs(11, [50] * 200))
    info, res = _lib.SortInfo(), _lib.TwobitResult()
    buf = np.frombuffer(text, np.uint8)
    for max_bytes, ok in ((len(text) - 1, False), (len(text), True)):
        ctx.twobit_pack_begin(max_bytes=max_bytes)
        half = len(text) // 2
        assert ctx.L.hpn_twobit_pack_add(ctx.h, C.c_void_p(buf.ctypes.data), half, 0, C.byref(info)) == 0
        rc = ctx.L.hpn_twobit_pack_add(ctx.h, C.c_void_p(buf.ctypes.data + half), len(text) - half, 1, C.byref(info))
        if ok:
            assert rc == 0 and info.store_bytes == len(text)
            assert ctx.L.hpn_twobit_pack_finish(ctx.h, C.byref(res)) == 0 and res.n_records == 200
        else:
            assert rc == _lib.E_CAPACITY and str(len(text)).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
            assert ctx.L.hpn_twobit_pack_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    ctx.twobit_pack_begin()
    ctx.twobit_pack_add(text[:100])
    got = C.c_uint64(0)
    assert ctx.L.hpn_twobit_pack_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    assert ctx.L.hpn_twobit_pack_write(ctx.h, 0, None, 0, C.byref(got)) == _lib.E_STATE
    ctx.twobit_pack_add(text[100:], last=True)
    assert ctx.L.hpn_twobit_pack_add(ctx.h, C.c_void_p(buf.ctypes.data), 10, 0, C.byref(info)) == _lib.E_STATE
    res = ctx.twobit_pack_finish()
    assert ctx.L.hpn_twobit_pack_write(ctx.h, res.out_bytes + 1, None, 0, C.byref(got)) == _lib.E_ARG
    # a sort session of the same context is not disturbed
    ctx.sort_begin()
    ctx.sort_add(text, last=True)
    assert ctx.twobit_pack_output() == twobit_ref.pack(text)[0]
    assert ctx.sort_finish().n_records == 200
    for bad, flag in ((read_input("fastq/trunc.fq"), _lib.TEXT_PARTIAL), (read_input("fastq/longname.fq"), _lib.TEXT_LONG_LINE),
                      (b"@a\nAC\0T\n+\nIIII\n", _lib.TEXT_NUL), (b"@a\nACGT\n+\nIIII\n@b\n", _lib.TEXT_PARTIAL)):
        ctx.twobit_pack_begin()
        assert ctx.twobit_pack_add(bad, last=True).irregular & flag
        assert ctx.L.hpn_twobit_pack_finish(ctx.h, C.byref(_lib.TwobitResult())) == _lib.E_STATE


def test_pack_every_golden_input(ctx):
    seen = set()
    for case in SAME:
        if case["tool"] != "pack" or case["in"] is None or case["in"] in seen:
            continue
        data = read_input(case["in"])
        if b"\0" in data:      # (irregular to the ABI; the tool frames it on the host)
            continue
        seen.add(case["in"])
        out, res = run_pack(ctx, data)
        stdout, files, _ = expected(case)
        assert out == (stdout or next(iter(files.values()), b""))
        check_outputs(case, *((out, {}) if not case["outputs"] else (b"", {case["outputs"][0]["name"]: out})))
    assert len(seen) >= 30


# ---- the ABI: unpack ----------------------------------------------------------------------------------------------

SEQLENS = list(range(21)) + [63, 64, 65, 150, 255]


def packed_lens(seqlen):
    m = (seqlen + 3) >> 2
    return sorted({p for p in (m, 1, m - 1, m + 1, 255) if 1 <= p <= 255})


@pytest.mark.parametrize("n", [0, 1, 2, 17, 4097])
def test_unpack_grid_host_pointers(ctx, n):
    rs = np.random.RandomState(20 + n)
    body = rs.randint(0, 256, max(n, 1) * 255).astype(np.uint8)
    for seqlen in SEQLENS:
        for plen in packed_lens(seqlen):
            packed = body[:n * plen]
            got = ctx.twobit_unpack(seqlen, plen, packed if n else np.zeros(1, np.uint8), n)
            assert got == twobit_ref.unpack_records(seqlen, plen, packed.tobytes(), n), (seqlen, plen, n)


def test_unpack_device_pointers_any_alignment(ctx):
    import torch
    rs = np.random.RandomState(31)
    for seqlen in (0, 7, 16, 150, 255):
        for plen in packed_lens(seqlen)[:3]:
            for n, shift_in, shift_out in ((1, 0, 0), (17, 3, 1), (300, 5, 8), (2, 1, 13)):
                packed = rs.randint(0, 256, n * plen).astype(np.uint8)
                d_in = torch.zeros(n * plen + 16, dtype=torch.uint8, device="cuda")
                d_in[shift_in:shift_in + n * plen] = torch.from_numpy(packed).cuda()
                need = n * (seqlen + 1)
                d_out = torch.full((need + 48,), 0xAA, dtype=torch.uint8, device="cuda")
                view = d_out[16 + shift_out:16 + shift_out + need]
                assert ctx.twobit_unpack(seqlen, plen, d_in[shift_in:], n, out=view) == need
                host = d_out.cpu().numpy()
                assert host[16 + shift_out:16 + shift_out + need].tobytes() == twobit_ref.unpack_records(seqlen, plen, packed.tobytes(), n), (seqlen, plen, n)
                assert (host[:16 + shift_out] == 0xAA).all() and (host[16 + shift_out + need:] == 0xAA).all()      # nothing in front, nothing behind


def test_unpack_errors(ctx):
    from highperformancengs_amd import _lib
    packed = np.arange(38 * 5, dtype=np.uint8)
    need = 5 * 151
    out = np.full(need, 0xAA, np.uint8)
    got = C.c_uint64(0)
    call = lambda seqlen, plen, n, cap: ctx.L.hpn_twobit_unpack(ctx.h, seqlen, plen, C.c_void_p(packed.ctypes.data), n, C.c_void_p(out.ctypes.data), cap, C.byref(got))
    assert call(150, 38, 5, need - 1) == _lib.E_CAPACITY and got.value == need and (out == 0xAA).all()      # the size needed; nothing written
    assert call(150, 0, 5, need) == _lib.E_ARG and (out == 0xAA).all()
    assert call(150, 0, 0, need) == 0 and got.value == 0      # no record: nothing to do, whatever the header says
    assert call(256, 38, 1, need) == _lib.E_ARG and call(150, 256, 1, need) == _lib.E_ARG
    assert call(150, 38, 5, need) == 0 and got.value == need
    assert out.tobytes() == twobit_ref.unpack_records(150, 38, packed.tobytes(), 5)


# ---- the tools ----------------------------------------------------------------------------------------------------

TOOL = {"pack": "fastq2twobit", "unpack": "twoBit2seq"}


def run_tool(case, cwd, env=None, path=None, data=None):
    """Runs a manifest case's tool in `cwd`.  path: another file than the case's input; data: bytes to put into a file first."""
    os.makedirs(cwd)
    if data is not None:
        path = os.path.join(str(cwd), "input.bin")
        open(path, "wb").write(data)
    path = path or (input_path(case["in"]) if case["in"] else None)
    cmd = [os.path.join(BIN, TOOL[case["tool"]])] + [path if a == "{in}" else a for a in case["args"]]
    kw = {"stdin": open(path, "rb") if case["stdin"] == "file" else subprocess.DEVNULL}
    p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    files = {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd) if fn != "input.bin"}
    files.pop("no_such_file.fq", None), files.pop("no_such_file.2bit", None)      # (a missing input is created, as the reference creates it)
    return p, files


def check_run(case, p, got, what):
    tool = TOOL[case["tool"]].encode()
    if case["expect"] == "refuse":
        assert p.returncode == 2 and p.stderr.startswith(tool + b": ") and p.stderr.count(b"\n") == 1, (what, p.returncode, p.stderr.decode("latin-1"))
        assert p.stdout == b"" and not any(got.values()), what
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
    data = case_input(case) if case["from"] else None
    p, got = run_tool(case, tmp_path / "r", data=data)
    check_run(case, p, got, "default")
    if case["tool"] == "pack" and case["in"] and case["expect"] != "usage":
        p, got = run_tool(case, tmp_path / "h", {"HPN_TEXT": "0"})      # framed on the host
        check_run(case, p, got, "host framer")
    if case["tool"] == "unpack" and case["expect"] == "same" and (case["in"] or case["from"]):
        p, got = run_tool(case, tmp_path / "c", {"HPN_TEXT_CHUNK": "64"}, data=data)      # the hooks build: a few records per chunk
        check_run(case, p, got, "small chunks")


@pytest.mark.parametrize("cid", ["p_syn_var_b_fq_gz", "p_multi_fq_gz", "p_mixed", "p_hi_mid"])
def test_fastq2twobit_on_every_route(cid, tmp_path):
    """The routes test_sort_gpu.py sends gzfastq_sort through, with the same switches of the hooks build."""
    case = BY_ID[cid]
    is_gz = case["in"].endswith(".gz")
    small = os.path.getsize(input_path(case["in"])) < 20000
    routes = [("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099", "HPN_TEXT_SLICE": "100" if small else "5000"})]
    if is_gz:
        routes += [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                   ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
                   ("host inflaters off", {"HPN_NO_MGZ": "1", "HPN_NO_PGZ": "1", "HPN_TEXT_CHUNK": "70001"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)
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


def test_twoBit2seq_chunk_borders(tmp_path):
    """seqlen 150, packedLen 38, 41 records and 37 bytes of a 42nd: with chunks of 64 bytes of input every chunk is one record, with
    100 bytes two, with 1,000 bytes 26 -- a border between records each time, the partial tail alone in (or at the end of) the last."""
    import twobit_inputs
    blob = twobit_inputs.twobit(150, 38, 41, 77, tail=b"\xe4" * 37)
    want = twobit_ref.unpack(blob)[0]
    assert len(want) == 41 * 151
    case = {"tool": "unpack", "in": None, "args": ["-i", "{in}", "-o", "o"], "stdin": None}
    for k, chunk in enumerate(("64", "100", "1000", str(38 * 41), str(38 * 41 + 37))):
        p, got = run_tool(case, tmp_path / ("c%d" % k), {"HPN_TEXT_CHUNK": chunk}, data=blob)
        assert p.returncode == 0 and got == {"o.decompress": want}, (chunk, p.stderr.decode("latin-1"))
    p, got = run_tool(dict(case, args=["-o", "-"], stdin="file"), tmp_path / "s", {"HPN_TEXT_CHUNK": "100"}, data=blob)
    assert p.returncode == 0 and p.stdout == want and got == {}


def test_round_trip_of_10000_reads(tmp_path):
    rs = np.random.RandomState(41)
    seqs = [bytes(x) for x in rs.choice(np.frombuffer(b"ACGT", np.uint8), (10_000, 150))]
    text = fastq(seqs)
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(text, 1))
    pack = {"tool": "pack", "in": None, "args": ["-i", "{in}", "-o", "o"], "stdin": None}
    p, got = run_tool(pack, tmp_path / "p", path=str(tmp_path / "a.fq.gz"))
    assert p.returncode == 0, p.stderr.decode("latin-1")
    assert got == {"o_sort_by_seq.fq": twobit_ref.pack(text)[0]} and len(got["o_sort_by_seq.fq"]) == 2 + 38 * 10_000
    assert "list count: 10000\n" in p.stderr.decode()
    unpack = {"tool": "unpack", "in": None, "args": ["-i", "{in}", "-o", "-"], "stdin": None}
    p, _ = run_tool(unpack, tmp_path / "u", path=str(tmp_path / "p" / "o_sort_by_seq.fq"))
    assert p.returncode == 0 and p.stdout == b"".join(s + b"\n" for s in reversed(seqs))
