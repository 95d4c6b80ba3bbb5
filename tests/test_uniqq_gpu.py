"""GPU: hpn_fastq_uniqq_* and bin/gzfastq_uniqQ against the reference's recorded outputs (tests/golden/uniqq/) and, on random
text, against the Python restatement that test_uniqq_golden.py pins to them."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import uniqq_ref
from test_uniq_gpu import cut_lists, random_reads
from test_uniqq_golden import CASES, GOLDEN, RUNS, by_count, check_recorded, expected, input_path, read_input, to_stdout

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def run_abi(ctx, data, cuts=None, hash_bits=0, slice_bytes=1 << 24, orders=(0, 1)):
    """({order: bytes}, result); order 0 = HPN_UNIQQ_KEY_ORDER (-S), 1 = HPN_UNIQQ_COUNT_ORDER (-C)."""
    ctx.uniqq_begin(hash_bits=hash_bits)
    a, n = 0, 0
    cuts = cuts or [len(data)]
    for c in cuts:
        info = ctx.uniqq_add(data[a:c], last=(c == cuts[-1]))
        assert info.irregular == 0, info.irregular
        n += info.n_records
        a = c
    res = ctx.uniqq_finish()
    assert n == res.n_records
    out = {w: ctx.uniqq_output(w, slice_bytes) for w in orders}
    for text in out.values():
        assert len(text) == res.out_bytes
    return out, res


def check_against_ref(out, res, data):
    r = uniqq_ref.collapse(data)
    assert (res.n_records, res.n_unique, res.hash_size, res.max_count) == (r.n, r.u, r.hash_size, r.max_count)
    for w, text in out.items():
        assert text == uniqq_ref.render(r, r.count_order if w else r.key_order), "-C" if w else "-S"
    return r


def with_short_qualities(text, seed):
    """Every fifth record's quality line cut to a random shorter length (0 included)."""
    rs = np.random.RandomState(seed)
    lines = text.split(b"\n")
    for i in range(3, len(lines) - 4, 20):      # (the last record keeps its line: without a final newline it loses a byte)
        lines[i] = lines[i][:int(rs.randint(0, len(lines[i]) + 1))]
    return b"\n".join(lines)


@pytest.mark.parametrize("final_newline", [True, False])
def test_abi_on_random_reads(ctx, final_newline):
    """~3,000 reads over ~400 keys of 0 .. 300 bytes, names and qualities of any length (short quality lines among them): one
    chunk, random cuts, one-byte chunks, a cut inside every line of the first records."""
    text = with_short_qualities(random_reads(150 + final_newline, 3000, 400, final_newline), 7)
    for cuts in cut_lists(13, len(text), text):
        out, res = run_abi(ctx, text, cuts=cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 100000)
        r = check_against_ref(out, res, text)
    assert 300 < r.u <= 400 and r.n == 3000 and out[0] != out[1]
    assert any(len(q) + 1 < len(k) for k, m in r.members.items() for n, q in m)


def grouping_hash(key):
    """The 64-bit grouping hash of kernels/fastq_uniq.hip (k_uniq_keys, k_uniq_pair): seed 1, base kUniqBase, modulo 2^64."""
    h = 1
    for c in key:
        h = (h * 0x9E3779B97F4A7C15 + c) & 0xFFFFFFFFFFFFFFFF
    return h


def span_text(n):
    """n records in random file order whose place in the order sorted by grouping hash is chosen: distinct 20-mers are ranked by
    their hash and given their multiplicities in that order -- singletons, one group of n // 2 members that spans whole tiles of
    the scan (2048 items), and a group of three at the sorted positions 2046 .. 2048 (n >= 2049: across the border of the first
    two tiles), else at the very end of the order (n = 2048: it ends on the border)."""
    rs = np.random.RandomState(n)
    big, singles = n // 2, n - n // 2 - 3
    keys = sorted({bytes(x) for x in rs.choice(np.frombuffer(b"ACGT", np.uint8), (singles + 2, 20))}, key=grouping_hash)
    assert len(keys) == singles + 2
    if singles + big <= 2046:
        counts = [1] * singles + [big, 3]
    else:
        counts = [1] * 2046 + [3, big] + [1] * (singles - 2046)
    assert sum(counts) == n and (n < 2049 or sum(counts[:counts.index(3)]) == 2046)
    which = [k for k, c in zip(keys, counts) for _ in range(c)]
    recs = [(b"@s%d" % j, which[i], bytes(rs.randint(33, 127, int(rs.randint(0, 50))).astype(np.uint8))) for j, i in enumerate(rs.permutation(n))]
    return b"".join(a + b"\n" + k + b"\n+\n" + q + b"\n" for a, k, q in recs)


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_scan_and_tile_edges(ctx, n):
    text = span_text(n)
    r = uniqq_ref.collapse(text)
    assert sorted(len(m) for m in r.members.values())[-2:] == [3, n // 2] and r.n == n
    for hash_bits in (0, 1):   # 0: the sorted order is span_text's; 1: two runs ordered by the keys' bytes
        out, res = run_abi(ctx, text, hash_bits=hash_bits)
        check_against_ref(out, res, text)
        assert hash_bits or res.hash_clashes == 0


def test_one_team_per_record_whatever_the_group(ctx):
    n = 100_000
    rs = np.random.RandomState(77)
    lens = rs.randint(0, 200, n)
    pool = rs.randint(33, 127, 400).astype(np.uint8).tobytes()
    same = b"".join(b"@s%d\nACGTACGTACGTACGTACGTAC\n+\n%s\n" % (i, pool[int(l):2 * int(l)]) for i, l in enumerate(lens))
    out, res = run_abi(ctx, same)
    r = check_against_ref(out, res, same)
    assert (r.u, r.n, res.max_count) == (1, n, n) and out[0] == out[1]
    seqs = set()
    while len(seqs) < n:
        seqs.update(bytes(x) for x in rs.choice(np.frombuffer(b"ACGT", np.uint8), (n, 30)))
    distinct = b"".join(b"@d%d\n%s\n+\n%s\n" % (i, s, b"I" * 30) for i, s in enumerate(sorted(seqs, key=lambda x: x[::-1])[:n]))
    out, res = run_abi(ctx, distinct)
    assert check_against_ref(out, res, distinct).u == n and res.max_count == 1
    out, res = run_abi(ctx, b"")
    assert (res.n_records, res.n_unique, res.hash_size, res.out_bytes, res.max_count, out) == (0, 0, 0, 0, 0, {0: b"", 1: b""})


def group_keys(text):
    """The sequences of a gzfastq_uniqQ output, group by group."""
    lines, keys, i = text.split(b"\n"), [], 0
    while i + 3 < len(lines):
        keys.append(lines[i + 1])
        i += 3 + int(lines[i].rsplit(b"\t", 1)[1])
    return keys


@pytest.mark.parametrize("u", [4, 5, 8, 9, 16, 17])
def test_equal_counts_come_in_the_order_of_the_table_walk(ctx, u):
    from highperformancengs_amd import _lib
    text = read_input("uniqq/inputs/equal_u%d.fq" % u)
    out, res = run_abi(ctx, text)
    assert (res.n_unique, res.max_count) == (u, 2)
    ctx.uniq_begin()
    ctx.uniq_add(text, last=True)
    ures = ctx.uniq_finish()
    table = ctx.uniq_output(_lib.UNIQ_TABLE_ORDER, 0)
    assert ures.hash_size == res.hash_size
    walk = table.split(b"\n")[1::4]
    assert len(walk) == u and group_keys(out[1]) == walk != group_keys(out[0])


ABI_CASES = [c for c in RUNS if c["expect"] == "same"]


@pytest.mark.parametrize("hash_bits", [8, 1])
@pytest.mark.parametrize("case", ABI_CASES, ids=[c["id"] for c in ABI_CASES])
def test_outputs_do_not_depend_on_the_hash_width(ctx, case, hash_bits):
    data = read_input(case["in1"])
    w = int(by_count(case))
    out, res = run_abi(ctx, data, hash_bits=hash_bits, orders=(w,))
    check_recorded(case, out[w])
    want, _, r = expected(case)
    assert out[w] == want
    assert (res.n_records, res.n_unique, res.hash_size) == (r.n, r.u, r.hash_size)
    if r.u > 2 and hash_bits == 1:
        assert res.hash_clashes > 0      # the byte comparison did the work


def test_write_in_slices_and_beyond_the_end(ctx):
    from highperformancengs_amd import _lib
    for text, slices in ((random_reads(172, 60, 9, max_len=40), (1,)), (random_reads(171, 600, 90, max_len=120), (4096, None))):
        whole, res = run_abi(ctx, text)
        assert res.out_bytes > (3 * 4096 if slices[0] == 4096 else 1000) and whole[0] != whole[1]
        for w in (_lib.UNIQQ_COUNT_ORDER, _lib.UNIQQ_KEY_ORDER):
            for slice_bytes in slices:
                assert ctx.uniqq_output(w, slice_bytes or res.out_bytes) == whole[w], (w, slice_bytes)
    got = C.c_uint64(7)
    buf = np.zeros(16, np.uint8)
    assert ctx.L.hpn_fastq_uniqq_write(ctx.h, 0, res.out_bytes, C.c_void_p(buf.ctypes.data), 16, C.byref(got)) == 0 and got.value == 0
    assert ctx.L.hpn_fastq_uniqq_write(ctx.h, 0, res.out_bytes + 1, C.c_void_p(buf.ctypes.data), 16, C.byref(got)) == _lib.E_ARG
    assert ctx.L.hpn_fastq_uniqq_write(ctx.h, 2, 0, C.c_void_p(buf.ctypes.data), 16, C.byref(got)) == _lib.E_ARG
    assert ctx.L.hpn_fastq_uniqq_write(ctx.h, 0, 0, None, 16, C.byref(got)) == _lib.E_ARG


def test_state_capacity_and_irregular_text(ctx):
    from highperformancengs_amd import _lib
    text = random_reads(181, 200, 50, max_len=80)
    info, res, got = _lib.UniqInfo(), _lib.UniqqResult(), C.c_uint64(0)
    buf = np.frombuffer(text, np.uint8)
    for max_bytes, ok in ((len(text) - 1, False), (len(text), True)):
        ctx.uniqq_begin(max_bytes=max_bytes)
        half = len(text) // 2
        assert ctx.L.hpn_fastq_uniqq_add(ctx.h, C.c_void_p(buf.ctypes.data), half, 0, C.byref(info)) == 0
        rc = ctx.L.hpn_fastq_uniqq_add(ctx.h, C.c_void_p(buf.ctypes.data + half), len(text) - half, 1, C.byref(info))
        if ok:
            assert rc == 0 and info.store_bytes == len(text)
            assert ctx.L.hpn_fastq_uniqq_finish(ctx.h, C.byref(res)) == 0 and res.n_records == 200
        else:
            assert rc == _lib.E_CAPACITY
            assert str(len(text)).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
            assert ctx.L.hpn_fastq_uniqq_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    # finish before the last chunk, write before finish, add behind the last chunk and behind finish, a hash width of 64
    ctx.uniqq_begin()
    ctx.uniqq_add(text[:100])
    assert ctx.L.hpn_fastq_uniqq_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    assert ctx.L.hpn_fastq_uniqq_write(ctx.h, 0, 0, C.c_void_p(buf.ctypes.data), 0, C.byref(got)) == _lib.E_STATE
    ctx.uniqq_add(text[100:], last=True)
    assert ctx.L.hpn_fastq_uniqq_add(ctx.h, C.c_void_p(buf.ctypes.data), 10, 0, C.byref(info)) == _lib.E_STATE
    ctx.uniqq_finish()
    assert ctx.L.hpn_fastq_uniqq_add(ctx.h, C.c_void_p(buf.ctypes.data), 10, 0, C.byref(info)) == _lib.E_STATE
    assert ctx.L.hpn_fastq_uniqq_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    assert ctx.L.hpn_fastq_uniqq_begin(ctx.h, 0, 64) == _lib.E_ARG
    # irregular text closes the session; a short quality line does not
    for bad, flag in ((read_input("fastq/trunc.fq"), _lib.TEXT_PARTIAL), (read_input("fastq/longname.fq"), _lib.TEXT_LONG_LINE),
                      (b"@a\nAC\0T\n+\nIIII\n", _lib.TEXT_NUL), (b"@a\nACGT\n+\nIIII\n@b\n", _lib.TEXT_PARTIAL)):
        ctx.uniqq_begin()
        info = ctx.uniqq_add(bad, last=True)
        assert info.irregular & flag, (bad[:20], info.irregular)
        assert ctx.L.hpn_fastq_uniqq_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    out, res = run_abi(ctx, b"@a\nACGT\n+\nII\n@b\nACGT\n+\nJ\n")
    assert out[0] == out[1] == b"@b\t2\nACGT\n+\nJ\nII\n"
    # a hpn_fastq_uniq session of the same context is another one
    ctx.uniq_begin()
    ctx.uniq_add(text, last=True)
    ctx.uniqq_begin()
    ctx.uniqq_add(text, last=True)
    assert ctx.uniq_finish().n_records == 200 == ctx.uniqq_finish().n_records


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, env=None, in1=None):
    in1 = in1 or input_path(case["in1"])
    os.makedirs(cwd)
    cmd = [os.path.join(BIN, "gzfastq_uniqQ")] + ([] if case["stdin"] else ["-1", in1]) + case["flags"] + (["-o", case["out"]] if case["out"] else [])
    with open(in1, "rb") if case["stdin"] else open(os.devnull, "rb") as stdin:
        p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p, {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd)}


def check_run(case, p, got, what):
    if case["expect"] == "refuse":
        assert p.returncode == 2 and b"gzfastq_uniqQ: " in p.stderr and p.stdout == b"" and got == {}, (what, p.returncode, p.stderr.decode("latin-1"))
        return
    assert p.returncode == 0, (what, p.stderr.decode("latin-1"))
    want, want_err, _ = expected(case)
    text = p.stdout if to_stdout(case) else got.get("o_sortKeyUniq.fq")
    assert text == want, what
    check_recorded(case, text, p.stdout, got)
    err = TIMES.sub("at T s", p.stderr.decode("latin-1"))
    assert err == want_err == case["stderr"], what


def bgzip(rel, path_out, block):
    from highperformancengs_amd.bamio import _Bgzf
    text = read_input(rel)
    with open(path_out, "wb") as fh:
        z = _Bgzf(fh)
        for i in range(0, len(text), block):
            z.write(text[i:i + block])
        z.close()


@pytest.mark.parametrize("case", RUNS, ids=[c["id"] for c in RUNS])
def test_tool_matches_the_reference_on_every_route(case, tmp_path):
    is_gz = case["in1"].endswith(".gz")
    small = os.path.getsize(input_path(case["in1"])) < 20000
    routes = [("default", {}), ("host framer", {"HPN_TEXT": "0"}),
              # the hooks build with forced small chunks and slices: records and output groups straddle many borders
              ("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099", "HPN_TEXT_SLICE": "100" if small else "5000"})]
    if is_gz:
        routes += [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                   ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
                   ("host inflaters off", {"HPN_NO_MGZ": "1", "HPN_NO_PGZ": "1", "HPN_TEXT_CHUNK": "70001"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)
    if case["expect"] == "refuse" and case["in1"].startswith("fastq/bad"):
        return      # (a damaged gzip stream cannot be re-packed)
    # the input re-packed as bgzip and as one gzip member under its own name (a file, or standard input)
    for kind in ("bgzip", "gzip"):
        packed = tmp_path / kind
        os.makedirs(packed)
        path = str(packed / os.path.basename(case["in1"]))
        if kind == "bgzip":
            bgzip(case["in1"], path, 3000 if small else 40000)
        else:
            open(path, "wb").write(gzip.compress(read_input(case["in1"]), 6))
        envs = [("bgzip, sliced", {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"})] if kind == "bgzip" else [("gzip copy on the device", {"HPN_GZ_GPU": "1"})]
        for k, (what, env) in enumerate(envs):
            p, got = run_tool(case, tmp_path / ("%s%d" % (kind, k)), env, path)
            check_run(case, p, got, what)


def test_tool_usage_nul_bytes_and_missing_files(tmp_path):
    os.makedirs(tmp_path / "w")
    exe = os.path.join(BIN, "gzfastq_uniqQ")
    assert {c["id"] for c in CASES if c["expect"] == "usage"} == {"no_arguments", "help"}
    for args in ([], ["-h"], ["-?"]):
        p = subprocess.run([exe] + args, cwd=tmp_path / "w", stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and b"Usage" in p.stderr and p.stdout == b""
    p = subprocess.run([exe, "-1", "no_such_file.fq", "-o", "x"], cwd=tmp_path / "w", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"no_such_file.fq" in p.stderr and p.stdout == b""
    (tmp_path / "nul.fq").write_bytes(b"@a\nACGT\n+\nIIII\n@b x\0y\nACGT\n+\nIIII\n")
    for env in ({}, {"HPN_TEXT": "0"}):
        p = subprocess.run([exe, "-1", str(tmp_path / "nul.fq"), "-C", "-o", "x"], cwd=tmp_path / "w", env={**os.environ, **env},
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2 and b"gzfastq_uniqQ: " in p.stderr and b"NUL" in p.stderr and p.stdout == b""
    assert os.listdir(tmp_path / "w") == []
