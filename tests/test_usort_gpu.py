"""GPU: hpn_fastq_usort_* and bin/gzfastq_uniq_sort against the reference's recorded outputs (tests/golden/usort/) and, on
random text, against the Python restatement that test_usort_golden.py pins to them."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import usort_ref
from test_uniq_gpu import cut_lists, random_reads
from test_uniqq_gpu import span_text
from test_usort_golden import BY_ID, RUNS, check_recorded, expected, input_path, out_prefix, read_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")
SUFFIX = ("_1_uniq.fq.gz", "_2_uniq.fq.gz")


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def feed(ctx, mate, data, cuts):
    a, n, bad = 0, 0, 0
    cuts = cuts or [len(data)]
    for c in cuts:
        info = ctx.usort_add(data[a:c], mate=mate, last=(c == cuts[-1]))
        if info.irregular:
            return n, info.irregular
        n += info.n_records
        a = c
    return n, bad


def run_abi(ctx, d1, d2=None, cuts1=None, cuts2=None, hash_bits=0, slice_bytes=1 << 24):
    """([mate 0's bytes, mate 1's], result); None where a chunk was irregular."""
    ctx.usort_begin(paired=d2 is not None, hash_bits=hash_bits)
    for mate, (d, cuts) in enumerate(((d1, cuts1), (d2, cuts2))):
        if d is not None and feed(ctx, mate, d, cuts)[1]:
            return None, None
    res = ctx.usort_finish()
    if res.no_answer:
        return None, res
    out = [ctx.usort_output(mate, slice_bytes) for mate in range(1 + (d2 is not None))]
    assert [len(t) for t in out] == list(res.out_bytes[:len(out)])
    return out, res


def check_against_ref(out, res, d1, d2=None):
    r = usort_ref.collapse(d1, d2)
    assert (res.n_records, res.n_unique, res.table_reads, res.hash_size, res.seq_len, res.max_count) == (r.n, r.u, r.e, r.hash_size, r.seq_len, r.max_count)
    assert res.unmatched == (r.error[0] if r.error else -1) and (not r.error or res.unmatched_name == r.error[1])
    for mate, text in enumerate(out):
        assert text == usort_ref.render(r, mate), "mate %d" % mate
    return r


def random_cuts(seed, n):
    rs = np.random.RandomState(seed)
    return sorted(set(int(x) for x in rs.randint(0, n + 1, 6)) | {n})


@pytest.mark.parametrize("case", RUNS, ids=[c["id"] for c in RUNS])
def test_recorded_runs_through_the_abi(ctx, case):
    try:
        d1, d2 = read_input(case["in1"]), read_input(case["in2"])
    except (zlib.error, gzip.BadGzipFile, EOFError):
        assert case["expect"] == "refuse"      # (a damaged gzip stream never reaches the ABI: the tool's test holds it)
        return
    if case["expect"] == "refuse":
        out, res = run_abi(ctx, d1, d2)
        assert out is None and (res is None or res.no_answer in (1, 2, 3))
        if case["id"] in ("pe_short_key", "pe_long_key", "e9"):
            assert res.no_answer == {"e9": 1, "pe_long_key": 2, "pe_short_key": 3}[case["id"]]
        return
    want, _, r = expected(case)
    names = [out_prefix(case) + s for s in SUFFIX]
    small = len(d1) < 1500
    variants = [dict(), dict(hash_bits=8), dict(hash_bits=1),
                dict(cuts1=random_cuts(1, len(d1)), cuts2=random_cuts(2, len(d2)) if d2 is not None else None, slice_bytes=4099)]
    if small:
        variants.append(dict(cuts1=list(range(1, len(d1) + 1)) or [0], cuts2=(list(range(1, len(d2) + 1)) or [0]) if d2 is not None else None))
    for kw in variants:
        out, res = run_abi(ctx, d1, d2, **kw)
        texts = dict(zip(names, out))
        assert texts == want, kw
        check_recorded(case, texts)
        assert (res.n_records, res.n_unique, res.table_reads, res.hash_size, res.seq_len) == (r.n, r.u, r.e, r.hash_size, r.seq_len)
        if kw.get("hash_bits") == 1 and r.u > 2:
            assert res.hash_clashes > 0      # the byte comparison did the work


def random_mates(seed, n, n_keys, lo, hi, names):
    """n mate-2 reads over n_keys sequences of lo .. hi bases."""
    rs = np.random.RandomState(seed)
    pool = [bytes(rs.choice(np.frombuffer(b"ACGTN", np.uint8), int(rs.randint(lo, hi + 1)))) for _ in range(n_keys)]
    out = []
    for i in range(n):
        s = pool[int(rs.randint(0, n_keys))]
        out.append(names(rs, i) + b"\n" + s + b"\n+\n" + bytes(rs.randint(33, 127, int(rs.randint(0, len(s) + 5))).astype(np.uint8)) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("final_newline", [True, False])
def test_abi_single_end_on_random_reads(ctx, final_newline):
    """~3,000 reads over ~400 keys of 0 .. 300 bytes, names and qualities of any length: one chunk, random cuts, one-byte
    chunks, a cut inside every line of the first records."""
    text = random_reads(250 + final_newline, 3000, 400, final_newline)
    for cuts in cut_lists(23, len(text), text):
        out, res = run_abi(ctx, text, cuts1=cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 100000)
        r = check_against_ref(out, res, text)
    assert 300 < r.u <= 400 and r.n == 3000
    assert any(len(k) < r.seq_len for k in r.first) and any(len(k) > r.seq_len for k in r.first)


@pytest.mark.parametrize("final_newline", [True, False])
def test_abi_pairs_on_random_reads(ctx, final_newline):
    """~3,000 pairs: mate 1 over keys of 0 .. 300 bytes, mate 2 over keys of 300 .. 340 -- every joined key reaches strLen, most
    mate-1 lines borrow from sequence 2 or leave a tail to the mate-2 line."""
    names = lambda tag: (lambda rs, i: b"@pair%d/x %s extra fields here" % (i, tag))
    t1 = random_reads(268 + final_newline, 3000, 40, final_newline, names=names(b"1"))
    t2 = random_mates(262, 3000, 10, 300, 340, names(b"2"))
    for c1, c2 in zip(cut_lists(24, len(t1), t1), cut_lists(25, len(t2), t2)):
        out, res = run_abi(ctx, t1, t2, c1, c2)
        r = check_against_ref(out, res, t1, t2)
    assert 300 < r.u <= 400 and r.n == 3000 and r.error is None
    lens = {len(rec1[1]) for _, rec1, _ in r.first.values()}
    assert min(lens) < r.seq_len < max(lens)
    # the mate file ends early / a name differs: reading stops there
    short2 = b"\n".join(t2.split(b"\n")[:4 * 1333]) + b"\n"
    out, res = run_abi(ctx, t1, short2)
    assert check_against_ref(out, res, t1, short2).error[0] == 1333
    lines = t2.split(b"\n")
    lines[4 * 2100] = b"@pair2100/y 2"
    out, res = run_abi(ctx, t1, b"\n".join(lines))
    assert check_against_ref(out, res, t1, b"\n".join(lines)).error[0] == 2100


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_scan_and_tile_edges(ctx, n):
    text = span_text(n)
    r = usort_ref.collapse(text)
    assert sorted(r.count.values())[-2:] == [3, n // 2] and r.n == n
    for hash_bits in (0, 1):   # 0: the sorted order is span_text's; 1: two runs ordered by the keys' bytes
        out, res = run_abi(ctx, text, hash_bits=hash_bits)
        check_against_ref(out, res, text)
        assert hash_bits or res.hash_clashes == 0


@pytest.mark.parametrize("u", [2047, 2048, 2049])
def test_equal_counts_rest_on_slot_and_first_ordinal(ctx, u):
    rs = np.random.RandomState(900 + u)
    keys = set()
    while len(keys) < u:
        keys.update(bytes(x) for x in rs.choice(np.frombuffer(b"ACGT", np.uint8), (u, 14)))
    keys = sorted(keys)[:u]
    idx = np.concatenate([rs.permutation(u), rs.permutation(u)])
    text = b"".join(b"@t%d\n%s\n+\n%s\n" % (i, keys[k], b"I" * (i % 15)) for i, k in enumerate(idx))
    r = usort_ref.collapse(text)
    assert set(r.count.values()) == {2} and r.u == u
    slots = [usort_ref.djb2_64(k) % r.hash_size for k in r.order]
    assert slots == sorted(slots) and len(set(slots)) < u      # chains of two and more: newest first decides inside them
    out, res = run_abi(ctx, text)
    check_against_ref(out, res, text)


def test_one_group_and_all_groups_of_100000(ctx):
    n = 100_000
    rs = np.random.RandomState(78)
    lens = rs.randint(0, 200, n)
    pool = rs.randint(33, 127, 400).astype(np.uint8).tobytes()
    same = b"".join(b"@s%d\nACGTACGTACGTACGTACGTAC\n+\n%s\n" % (i, pool[int(l):2 * int(l)]) for i, l in enumerate(lens))
    out, res = run_abi(ctx, same)
    r = check_against_ref(out, res, same)
    assert (r.u, r.n, res.max_count) == (1, n, n) and out[0].startswith(b"@s0\t100000\n")
    seqs = set()
    while len(seqs) < n:
        seqs.update(bytes(x) for x in rs.choice(np.frombuffer(b"ACGT", np.uint8), (n, 30)))
    distinct = b"".join(b"@d%d\n%s\n+\n%s\n" % (i, s, b"I" * 30) for i, s in enumerate(sorted(seqs, key=lambda x: x[::-1])[:n]))
    out, res = run_abi(ctx, distinct)
    assert check_against_ref(out, res, distinct).u == n and res.max_count == 1 and res.hash_size == 134000
    out, res = run_abi(ctx, b"")
    assert (res.n_records, res.n_unique, res.table_reads, res.hash_size, list(res.out_bytes), res.max_count, out) == (0, 0, 0, 0, [0, 0], 0, [b""])


def test_write_in_slices_state_and_errors(ctx):
    from highperformancengs_amd import _lib
    text = random_reads(271, 600, 90, max_len=120)
    whole, res = run_abi(ctx, text)
    assert res.out_bytes[0] > 3 * 4096
    for slice_bytes in (4096, res.out_bytes[0]):
        assert ctx.usort_output(0, slice_bytes) == whole[0]
    got, info, rs_, buf = C.c_uint64(7), _lib.UniqInfo(), _lib.UsortResult(), np.zeros(16, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert ctx.L.hpn_fastq_usort_write(ctx.h, 0, res.out_bytes[0], p, 16, C.byref(got)) == 0 and got.value == 0
    assert ctx.L.hpn_fastq_usort_write(ctx.h, 0, res.out_bytes[0] + 1, p, 16, C.byref(got)) == _lib.E_ARG
    assert ctx.L.hpn_fastq_usort_write(ctx.h, 1, 0, p, 16, C.byref(got)) == _lib.E_ARG      # mate 1 of a single-end session
    assert ctx.L.hpn_fastq_usort_write(ctx.h, 0, 0, None, 16, C.byref(got)) == _lib.E_ARG
    assert ctx.L.hpn_fastq_usort_add(ctx.h, 0, p, 10, 0, C.byref(info)) == _lib.E_STATE      # behind finish
    assert ctx.L.hpn_fastq_usort_finish(ctx.h, C.byref(rs_)) == _lib.E_STATE
    assert ctx.L.hpn_fastq_usort_begin(ctx.h, 0, 0, 64) == _lib.E_ARG
    raw = np.frombuffer(text, np.uint8)
    for max_bytes, ok in ((len(text) - 1, False), (len(text), True)):
        ctx.usort_begin(max_bytes=max_bytes)
        rc = ctx.L.hpn_fastq_usort_add(ctx.h, 0, C.c_void_p(raw.ctypes.data), len(text), 1, C.byref(info))
        assert rc == (0 if ok else _lib.E_CAPACITY)
        assert ctx.L.hpn_fastq_usort_finish(ctx.h, C.byref(rs_)) == (0 if ok else _lib.E_STATE)
    ctx.usort_begin(paired=True)
    ctx.usort_add(text, mate=0, last=True)
    assert ctx.L.hpn_fastq_usort_finish(ctx.h, C.byref(rs_)) == _lib.E_STATE      # mate 1 has not had its last chunk
    assert ctx.L.hpn_fastq_usort_write(ctx.h, 0, 0, p, 0, C.byref(got)) == _lib.E_STATE
    # irregular text closes the session; a refusal of finish leaves no output; sessions of the siblings are others
    for bad, flag in ((read_input("fastq/trunc.fq"), _lib.TEXT_PARTIAL), (read_input("fastq/longname.fq"), _lib.TEXT_LONG_LINE),
                      (b"@a\nAC\0T\n+\nIIII\n", _lib.TEXT_NUL)):
        ctx.usort_begin()
        assert ctx.usort_add(bad, last=True).irregular & flag
        assert ctx.L.hpn_fastq_usort_finish(ctx.h, C.byref(rs_)) == _lib.E_STATE
    ctx.usort_begin()
    ctx.usort_add(b"@a\nACGT\n+\nIIII\n", last=True)
    assert ctx.L.hpn_fastq_usort_finish(ctx.h, C.byref(rs_)) == _lib.E_DOMAIN and rs_.no_answer == _lib.USORT_FEW_READS
    assert b"divides" in ctx.L.hpn_ctx_last_error(ctx.h)
    assert ctx.L.hpn_fastq_usort_write(ctx.h, 0, 0, p, 16, C.byref(got)) == _lib.E_STATE
    ctx.uniq_begin()
    ctx.uniq_add(text, last=True)
    ctx.usort_begin()
    ctx.usort_add(text, last=True)
    assert ctx.uniq_finish().n_records == 600 == ctx.usort_finish().n_records


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, env=None, files=None):
    """files: {local name: path} to use in place of the case's inputs."""
    os.makedirs(cwd)
    placed = []
    for rel, name in ((case["in1"], case["name1"]), (case["in2"], case["name2"])):
        if rel:
            shutil.copy((files or {}).get(name) or input_path(rel), os.path.join(cwd, name))
            placed.append(name)
    cmd = [os.path.join(BIN, "gzfastq_uniq_sort")] + [a.replace("{1}", case["name1"] or "").replace("{2}", case["name2"] or "") for a in case["args"]]
    p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p, {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd) if fn not in placed}


def check_run(case, p, got, what):
    if case["expect"] == "refuse":
        assert p.returncode == 2 and b"gzfastq_uniq_sort: " in p.stderr and p.stdout == b"" and got == {}, (what, p.returncode, p.stderr.decode("latin-1"))
        return
    assert p.returncode == 0 and p.stdout == b"", (what, p.stderr.decode("latin-1"))
    want, want_err, _ = expected(case)
    texts = {fn: gzip.decompress(raw) for fn, raw in got.items()}
    assert texts == want, what
    check_recorded(case, texts)
    err = TIMES.sub("at T s", p.stderr.decode("latin-1"))
    assert err == want_err == case["stderr"], what


@pytest.mark.parametrize("case", RUNS, ids=[c["id"] for c in RUNS])
def test_tool_matches_the_reference(case, tmp_path):
    is_gz = any(rel and rel.endswith(".gz") for rel in (case["in1"], case["in2"]))
    small = os.path.getsize(input_path(case["in1"])) < 20000
    routes = [("default", {}), ("host framer", {"HPN_TEXT": "0"}),
              # the hooks build with forced small chunks and slices: records and output records straddle many borders
              ("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099", "HPN_TEXT_SLICE": "100" if small else "5000"})]
    if is_gz:
        routes += [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                   ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)


def bgzip(text, path_out, block):
    from highperformancengs_amd.bamio import _Bgzf
    with open(path_out, "wb") as fh:
        z = _Bgzf(fh)
        for i in range(0, len(text), block):
            z.write(text[i:i + block])
        z.close()


def test_tool_on_every_input_route(tmp_path):
    """One small paired input as plain text, one gzip member, several members and BGZF, the mates packed alike and unlike."""
    case = BY_ID["pairs_dups"]
    d = [read_input(case["in1"]), read_input(case["in2"])]
    packed = {}
    for k in (0, 1):
        name = case["name%d" % (k + 1)]
        os.makedirs(tmp_path / "in" / "plain", exist_ok=True)
        packed["plain", name] = str(tmp_path / "in" / "plain" / name)
        open(packed["plain", name], "wb").write(d[k])
        for kind in ("gzip", "multi", "bgzf"):
            os.makedirs(tmp_path / "in" / kind, exist_ok=True)
            path = packed[kind, name] = str(tmp_path / "in" / kind / name)
            if kind == "gzip":
                open(path, "wb").write(gzip.compress(d[k], 6))
            elif kind == "multi":
                cuts = [0, len(d[k]) // 3, len(d[k]) // 3 + 1, len(d[k]) * 3 // 4, len(d[k])]       # (cut anywhere, inside records)
                open(path, "wb").write(b"".join(gzip.compress(d[k][a:b], 6) for a, b in zip(cuts, cuts[1:])))
            else:
                bgzip(d[k], path, 3000)
    runs = [("plain", "plain", {}), ("gzip", "gzip", {"HPN_GZ_GPU": "1"}), ("gzip", "gzip", {"HPN_GZ_GPU": "0"}), ("multi", "multi", {}),
            ("bgzf", "bgzf", {}), ("bgzf", "bgzf", {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"}), ("bgzf", "plain", {}), ("gzip", "multi", {"HPN_GZ_GPU": "1"}),
            ("gzip", "gzip", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"})]
    for k, (kind1, kind2, env) in enumerate(runs):
        files = {case["name1"]: packed[kind1, case["name1"]], case["name2"]: packed[kind2, case["name2"]]}
        p, got = run_tool(case, tmp_path / ("run%d" % k), env, files)
        check_run(case, p, got, (kind1, kind2, env))


def test_tool_usage_missing_files_and_nul_bytes(tmp_path):
    os.makedirs(tmp_path / "w")
    exe = os.path.join(BIN, "gzfastq_uniq_sort")
    run = lambda args, env=None: subprocess.run([exe] + args, cwd=tmp_path / "w", env={**os.environ, **(env or {})}, stdin=subprocess.DEVNULL,
                                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for args in ([], ["-h"], ["-?"]):
        p = run(args)
        assert p.returncode == 1 and b"Usage" in p.stderr and p.stdout == b""
    p = run(["-1", "no_such_file.fq", "-o", "x"])
    assert p.returncode == 2 and b"no_such_file.fq" in p.stderr and p.stdout == b""
    p = run(["-2", "no_such_file.fq", "-o", "x"])
    assert p.returncode == 2 and b"-1" in p.stderr
    ten = b"".join(b"@r%d\nACGT\n+\nIIII\n" % i for i in range(12))
    (tmp_path / "nul.fq").write_bytes(ten + b"@b x\0y\nACGT\n+\nIIII\n")
    for env in ({}, {"HPN_TEXT": "0"}):
        p = run(["-1", str(tmp_path / "nul.fq"), "-o", "x"], env)
        assert p.returncode == 2 and b"gzfastq_uniq_sort: " in p.stderr and b"NUL" in p.stderr and p.stdout == b""
    assert os.listdir(tmp_path / "w") == []
