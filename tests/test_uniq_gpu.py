"""GPU: hpn_fastq_uniq_*, the radix sort behind it and bin/gzfastq_uniq against the reference's recorded outputs
(tests/golden/uniq/) and, on random text, against the Python restatement that test_uniq_golden.py pins to them."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import uniq_ref
from test_uniq_golden import CASES, GOLDEN, check_outputs, expected_files, input_path, read_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def feed(ctx, mate, text, cuts):
    a, n = 0, 0
    for c in cuts:
        info = ctx.uniq_add(text[a:c], mate=mate, last=(c == cuts[-1]))
        assert info.irregular == 0, info.irregular
        n += info.n_records
        a = c
    return n


def run_abi(ctx, data1, data2=None, cuts1=None, cuts2=None, hash_bits=0, slice_bytes=1 << 24):
    from highperformancengs_amd import _lib
    ctx.uniq_begin(paired=data2 is not None, hash_bits=hash_bits)
    feed(ctx, 0, data1, cuts1 or [len(data1)])
    if data2 is not None:
        feed(ctx, 1, data2, cuts2 or [len(data2)])
    res = ctx.uniq_finish()
    if data2 is None:
        out = {"_uniq.fq": ctx.uniq_output(_lib.UNIQ_TABLE_ORDER, 0, slice_bytes), "_sortKeyUniq.fq": ctx.uniq_output(_lib.UNIQ_KEY_ORDER, 0, slice_bytes)}
        assert len(out["_uniq.fq"]) == len(out["_sortKeyUniq.fq"]) == res.out_bytes[0]
    else:
        out = {"_1_uniq.fq": ctx.uniq_output(_lib.UNIQ_TABLE_ORDER, 0, slice_bytes), "_2_uniq.fq": ctx.uniq_output(_lib.UNIQ_TABLE_ORDER, 1, slice_bytes)}
        assert (len(out["_1_uniq.fq"]), len(out["_2_uniq.fq"])) == (res.out_bytes[0], res.out_bytes[1])
    return out, res


def check_against_ref(out, res, data1, data2=None):
    want, _, r = uniq_ref.simulate(data1, data2)
    assert (res.n_records, res.n_unique, res.hash_size) == (r.n, r.u, r.hash_size)
    assert res.unmatched == (r.error[0] if r.error else -1)
    if r.error:
        assert res.unmatched_name == r.error[1]
    assert out == want
    return r


def random_reads(seed, n, n_keys, final_newline=True, max_len=300, names=None):
    """n reads drawn from n_keys sequences of 0 .. max_len bytes (any byte but '\\n' and NUL in a tenth of them), qualities
    of the sequence's length (a few longer, a few one byte shorter), names of 1 .. 300 bytes with high bytes."""
    rs = np.random.RandomState(seed)
    pool = []
    for k in range(n_keys):
        ln = int(rs.choice([0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257])) if rs.rand() < 0.3 else int(rs.randint(0, max_len + 1))
        ln = min(ln, max_len)
        if rs.rand() < 0.1:
            s = rs.randint(1, 256, ln).astype(np.uint8)
            s[s == 10] = 65
        else:
            s = rs.choice(np.frombuffer(b"ACGTN", np.uint8), ln)
        pool.append(s.tobytes())
    out = []
    for i in range(n):
        s = pool[int(rs.randint(0, n_keys))]
        ql = len(s) if rs.rand() < 0.8 else (len(s) + int(rs.randint(0, 20)) if rs.rand() < 0.7 else max(len(s) - 1, 0))
        if i == n - 1 and not final_newline:
            ql = len(s) + 1      # (the last line without its newline loses a byte)
        qual = rs.randint(33, 127, ql).astype(np.uint8).tobytes()
        if names:
            name = names(rs, i)
        else:
            nm = rs.randint(1, 256, int(rs.randint(1, 301))).astype(np.uint8)
            nm[nm == 10] = 32
            nm[0] = ord("@")
            name = nm.tobytes()
        plus = b"+" if rs.rand() < 0.8 else b"+" + name[1:30]
        out.append(name + b"\n" + s + b"\n" + plus + b"\n" + qual + b"\n")
    text = b"".join(out)
    return text if final_newline else text[:-1]


def cut_lists(seed, n, text=None):
    rs = np.random.RandomState(seed)
    few = sorted(set(int(x) for x in rs.randint(0, n + 1, 7)) | {n})
    ones = sorted(set(range(1, min(n, 900))) | set(int(x) for x in rs.randint(0, n + 1, 5)) | {n})   # 1-byte chunks, then a few large ones
    lists = [[n], few, ones]
    if text is not None:   # a cut inside every line (and at every line's end) of the first records
        nl = [i for i in range(min(n, 6000)) if text[i] == 10]
        inside = sorted(set((a + b) // 2 for a, b in zip([0] + nl, nl)) | set(nl) | {n})
        lists.append(inside)
    return lists


@pytest.mark.parametrize("final_newline", [True, False])
def test_abi_single_end_on_random_text(ctx, final_newline):
    text = random_reads(50 + final_newline, 900, 200, final_newline)
    for cuts in cut_lists(3, len(text), text):
        out, res = run_abi(ctx, text, cuts1=cuts, slice_bytes=1 << 24 if len(cuts) < 50 else 1000)
        r = check_against_ref(out, res, text)
    assert 0 < r.u < r.n == 900


def test_abi_pairs_on_random_text(ctx):
    names = lambda tag: (lambda rs, i: b"@pair%d/x %s extra fields here" % (i, tag))
    t1 = random_reads(61, 700, 40, max_len=60, names=names(b"1"))
    t2 = random_reads(62, 700, 6, max_len=60, names=names(b"2"))
    for c1, c2 in zip(cut_lists(4, len(t1), t1), cut_lists(5, len(t2), t2)):
        out, res = run_abi(ctx, t1, t2, c1, c2)
        r = check_against_ref(out, res, t1, t2)
    assert 0 < r.u < r.n == 700
    # the mate file ends early / a name differs: reading stops there
    short2 = b"\n".join(t2.split(b"\n")[:4 * 333]) + b"\n"
    out, res = run_abi(ctx, t1, short2)
    assert check_against_ref(out, res, t1, short2).error[0] == 333
    bad2 = t2.replace(b"@pair500/x", b"@pair5oo/x")
    out, res = run_abi(ctx, t1, bad2)
    assert check_against_ref(out, res, t1, bad2).error[0] == 500
    out, res = run_abi(ctx, short2, t1)      # mate 0 is the shorter one: no error
    assert check_against_ref(out, res, short2, t1).error is None and res.n_records == 333


def test_abi_names_of_three_and_more_fields(ctx):
    names = lambda rs, i: b"@SRR%d.%d %d length=%d extra=%s" % (int(rs.randint(1, 99)), i, i, int(rs.randint(1, 300)), b" ".join([b"f"] * int(rs.randint(0, 9))))
    text = random_reads(71, 500, 60, names=names)
    out, res = run_abi(ctx, text)
    r = check_against_ref(out, res, text)
    assert 0 < r.u < r.n


def test_abi_all_identical_all_distinct_and_empty(ctx):
    same = b"".join(b"@s%d\nACGTACGTACGTACGTACGTAC\n+\n%s\n" % (i, bytes([33 + (i * 7) % 60]) * 22) for i in range(20000))
    out, res = run_abi(ctx, same)
    r = check_against_ref(out, res, same)
    assert (r.u, r.n) == (1, 20000)
    rs = np.random.RandomState(9)
    seqs = set()
    while len(seqs) < 20000:
        seqs.add(bytes(rs.choice(np.frombuffer(b"ACGT", np.uint8), 30)))
    distinct = b"".join(b"@d%d\n%s\n+\n%s\n" % (i, s, b"I" * 30) for i, s in enumerate(sorted(seqs, key=lambda x: x[::-1])))
    out, res = run_abi(ctx, distinct)
    assert check_against_ref(out, res, distinct).u == 20000
    out, res = run_abi(ctx, b"")
    assert (res.n_records, res.n_unique, res.hash_size, out) == (0, 0, 0, {"_uniq.fq": b"", "_sortKeyUniq.fq": b""})


def test_abi_a_million_reads_with_duplicates(ctx):
    rs = np.random.RandomState(12)
    n, n_keys = 1_000_000, 700_000      # ~30 % of the reads repeat an earlier sequence
    pool = rs.choice(np.frombuffer(b"ACGT", np.uint8), (n_keys, 50))
    pick = np.concatenate([np.arange(n_keys), rs.randint(0, n_keys, n - n_keys)])
    rs.shuffle(pick)
    qual = rs.randint(33, 74, (n, 50)).astype(np.uint8)
    seqs = [bytes(x) for x in pool[pick]]
    quals = [bytes(x) for x in qual]
    text = b"".join(b"@read%d\n%s\n+\n%s\n" % (i, seqs[i], quals[i]) for i in range(n))
    cuts = list(range(8 << 20, len(text), 8 << 20)) + [len(text)]
    out, res = run_abi(ctx, text, cuts1=cuts, slice_bytes=4 << 20)
    r = check_against_ref(out, res, text)
    assert r.n == n and 0.65 * n < r.u < 0.75 * n
    assert res.hash_clashes == 0


def test_abi_capacity_and_state(ctx):
    from highperformancengs_amd import _lib
    text = random_reads(81, 200, 50, max_len=80)
    info, res = _lib.UniqInfo(), _lib.UniqResult()
    buf = np.frombuffer(text, np.uint8)
    for max_bytes, ok in ((len(text) - 1, False), (len(text), True)):
        ctx.uniq_begin(max_bytes=max_bytes)
        half = len(text) // 2
        assert ctx.L.hpn_fastq_uniq_add(ctx.h, 0, C.c_void_p(buf.ctypes.data), half, 0, C.byref(info)) == 0
        rc = ctx.L.hpn_fastq_uniq_add(ctx.h, 0, C.c_void_p(buf.ctypes.data + half), len(text) - half, 1, C.byref(info))
        if ok:
            assert rc == 0 and info.store_bytes == len(text)
            assert ctx.L.hpn_fastq_uniq_finish(ctx.h, C.byref(res)) == 0 and res.n_records == 200
        else:
            assert rc == _lib.E_CAPACITY
            assert str(len(text)).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
            assert ctx.L.hpn_fastq_uniq_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    # finish before the last chunk, a mate a single-end session does not have, the sorted output of a paired session
    ctx.uniq_begin()
    ctx.uniq_add(text[:100])
    assert ctx.L.hpn_fastq_uniq_finish(ctx.h, C.byref(res)) == _lib.E_STATE
    assert ctx.L.hpn_fastq_uniq_add(ctx.h, 1, C.c_void_p(buf.ctypes.data), 10, 0, C.byref(info)) == _lib.E_ARG
    ctx.uniq_begin(paired=True)
    ctx.uniq_add(text, mate=0, last=True)
    ctx.uniq_add(text, mate=1, last=True)
    ctx.uniq_finish()
    got = C.c_uint64(0)
    assert ctx.L.hpn_fastq_uniq_write(ctx.h, _lib.UNIQ_KEY_ORDER, 0, 0, None, 0, C.byref(got)) == _lib.E_ARG


def test_abi_reports_irregular_text(ctx):
    from highperformancengs_amd import _lib
    for text, flag in ((read_input("fastq/trunc.fq"), _lib.TEXT_PARTIAL), (read_input("fastq/longname.fq"), _lib.TEXT_LONG_LINE),
                       (b"@a\nAC\0T\n+\nIIII\n", _lib.TEXT_NUL), (read_input("uniq/inputs/shortq.fq"), _lib.TEXT_SHORT_QUAL),
                       (b"@a\nACGT\n+\nIIII\n@b\n", _lib.TEXT_PARTIAL)):
        ctx.uniq_begin()
        info = ctx.uniq_add(text, last=True)
        assert info.irregular & flag, (text[:20], info.irregular)
    # more than one line per four bytes is regular here
    dense = b"@\n\n+\n\n" * 5000 + b"@\nA\n+\n!\n" * 3
    out, res = run_abi(ctx, dense)
    check_against_ref(out, res, dense)


# (text with NUL bytes is irregular to the ABI -- test_abi_reports_irregular_text; the tool frames it on the host, below)
ABI_CASES = [c for c in CASES if c["expect"] != "refuse" and b"\0" not in read_input(c["in1"])]


@pytest.mark.parametrize("hash_bits", [8, 1])
@pytest.mark.parametrize("case", ABI_CASES, ids=[c["id"] for c in ABI_CASES])
def test_outputs_do_not_depend_on_the_hash_width(ctx, case, hash_bits):
    d1 = read_input(case["in1"])
    d2 = read_input(case["in2"]) if case["in2"] else None
    out, res = run_abi(ctx, d1, d2, hash_bits=hash_bits)
    check_outputs(case, {"o" + k: v for k, v in out.items()})
    want, _, r = expected_files(case)
    assert {"o" + k: v for k, v in out.items()} == want
    assert (res.n_records, res.n_unique, res.hash_size) == (r.n, r.u, r.hash_size)
    if r.u > 2 and hash_bits == 1:
        assert res.hash_clashes > 0      # the byte comparison did the work


# ---- the radix sort -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2047, 2048, 2049, 1_000_003])
def test_radix_sort_against_numpy(ctx, n):
    rs = np.random.RandomState(n % 1000)
    vals = np.arange(n, dtype=np.uint32)
    sets = {"random": rs.randint(0, 1 << 62, n).astype(np.uint64) * np.uint64(4) + rs.randint(0, 4, n).astype(np.uint64),
            "all equal": np.full(n, 0xDEADBEEFCAFEF00D, np.uint64),
            "few": rs.randint(0, 3, n).astype(np.uint64) << np.uint64(40),
            "one digit": np.uint64(0x0102030405060708) ^ (rs.randint(0, 256, n).astype(np.uint64) << np.uint64(24)),
            "top digit": rs.randint(0, 256, n).astype(np.uint64) << np.uint64(56)}
    for what, keys in sets.items():
        k, v = ctx.sort_pairs(keys, vals)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(v, vals[order]), what
        assert np.array_equal(k, keys[order]), what


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, env=None, in1=None, in2=None):
    in1 = in1 or input_path(case["in1"])
    in2 = in2 or (input_path(case["in2"]) if case["in2"] else None)
    os.makedirs(cwd)
    p = subprocess.run([os.path.join(BIN, "gzfastq_uniq"), "-1", in1] + (["-2", in2] if in2 else []) + (["-o", "o"] if case["out"] else []), cwd=cwd,
                       env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p, {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd)}


def check_run(case, p, got, what):
    if case["expect"] == "refuse":
        assert p.returncode == 2 and b"gzfastq_uniq: " in p.stderr, (what, p.returncode, p.stderr.decode("latin-1"))
        return
    assert p.returncode == 0, (what, p.stderr.decode("latin-1"))
    assert p.stdout == b""
    check_outputs(case, got)
    want, want_err, _ = expected_files(case)
    assert got == want, what
    err = TIMES.sub("at T s", p.stderr.decode("latin-1"))
    assert err == want_err, what
    if case["expect"] == "same":
        assert err == case["stderr"], what


def bgzip(rel, path_out, block):
    from highperformancengs_amd.bamio import _Bgzf
    text = read_input(rel)
    with open(path_out, "wb") as fh:
        z = _Bgzf(fh)
        for i in range(0, len(text), block):
            z.write(text[i:i + block])
        z.close()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tool_matches_the_reference_on_every_route(case, tmp_path):
    is_gz = case["in1"].endswith(".gz") or bool(case["in2"] and case["in2"].endswith(".gz"))
    small = os.path.getsize(input_path(case["in1"])) < 20000
    routes = [("default", {}), ("host framer", {"HPN_TEXT": "0"}),
              # the hooks build with forced small chunks and slices: records and output records straddle many borders
              ("small chunks", {"HPN_TEXT_CHUNK": "64" if small else "4099", "HPN_TEXT_SLICE": "100" if small else "5000"})]
    if is_gz:
        routes += [("gzip on the device", {"HPN_GZ_GPU": "1"}), ("gzip on the host", {"HPN_GZ_GPU": "0"}),
                   ("gzip on the device, small stretches", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
                   ("host inflaters off", {"HPN_NO_MGZ": "1", "HPN_NO_PGZ": "1", "HPN_TEXT_CHUNK": "70001"})]
    for k, (what, env) in enumerate(routes):
        p, got = run_tool(case, tmp_path / ("r%d" % k), env)
        check_run(case, p, got, what)
    if case["expect"] == "refuse" and (case["in1"].startswith("fastq/bad") or not case["out"]):
        return      # (a damaged gzip stream cannot be re-packed)
    # the inputs re-packed as bgzip and as one gzip member under their own names
    for kind in ("bgzip", "gzip"):
        packed = tmp_path / kind
        os.makedirs(packed)
        ins = []
        for rel in (case["in1"], case["in2"]):
            if not rel:
                ins.append(None)
                continue
            ins.append(str(packed / os.path.basename(rel)))
            if kind == "bgzip":
                bgzip(rel, ins[-1], 3000 if small else 40000)
            else:
                open(ins[-1], "wb").write(gzip.compress(read_input(rel), 6))
        envs = [("bgzip, sliced", {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"})] if kind == "bgzip" else [("gzip copy on the device", {"HPN_GZ_GPU": "1"})]
        for k, (what, env) in enumerate(envs):
            p, got = run_tool(case, tmp_path / ("%s%d" % (kind, k)), env, ins[0], ins[1])
            check_run(case, p, got, what)


def test_tool_usage_errors(tmp_path):
    os.makedirs(tmp_path / "w")
    exe = os.path.join(BIN, "gzfastq_uniq")
    t = os.path.join(GOLDEN, "fastq", "t.fq")
    p = subprocess.run([exe], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"Usage" in p.stderr
    p = subprocess.run([exe, "-h"], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"Usage" in p.stderr
    p = subprocess.run([exe, "-o", "x"], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"-1" in p.stderr
    p = subprocess.run([exe, "-1", "no_such_file.fq", "-o", "x"], cwd=tmp_path / "w", stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"no_such_file.fq" in p.stderr
    for extra in ([], ["-o", "-"], ["-o", "-x"]):
        p = subprocess.run([exe, "-1", t] + extra, cwd=tmp_path / "w", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2 and b"gzfastq_uniq: " in p.stderr and p.stdout == b""
    assert os.listdir(tmp_path / "w") == []


def test_tool_on_larger_files_with_many_chunks(tmp_path):
    """~30 MB of text per mate (several chunks and slices on every route), single-end and paired, names of four fields."""
    names = lambda tag: (lambda rs, i: b"@SRR7.%d %d/%s length=60" % (i, i, tag))
    t1 = random_reads(91, 4000, 900, max_len=120, names=names(b"1")) * 40
    t2 = random_reads(92, 4000, 30, max_len=120, names=names(b"2")) * 40
    (tmp_path / "a_1.fq.gz").write_bytes(gzip.compress(t1, 1))
    (tmp_path / "a_2.fq").write_bytes(t2)
    for in2, d2 in ((None, None), (str(tmp_path / "a_2.fq"), t2)):
        want, want_err, r = uniq_ref.simulate(t1, d2)
        assert 0 < r.u < r.n
        case = {"in1": None, "in2": None, "out": True}
        for k, env in enumerate(({}, {"HPN_GZ_GPU": "1"}, {"HPN_TEXT": "0"})):
            p, got = run_tool(case, tmp_path / ("r%d%d" % (k, in2 is not None)), env, str(tmp_path / "a_1.fq.gz"), in2)
            assert p.returncode == 0, p.stderr.decode("latin-1")
            assert got == {"o" + k2: v for k2, v in want.items()} and TIMES.sub("at T s", p.stderr.decode("latin-1")) == want_err
