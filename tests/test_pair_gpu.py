"""GPU: hpn_fastq_pair_* and bin/pick_pair against the reference's recorded runs (tests/golden/pair/) and, on inputs that are not
recorded, against the Python restatement that test_pair_golden.py pins to them.  The ROUTE is part of every assertion: the session's
`route` / `unverified` and the tool's HPN_TIMING line must be what pair_ref's certificate predicts, in both directions -- a wrong
join must not hide behind the host's walk, and the host's walk must not hide a join that should have verified."""
import gzip
import os
import re
import subprocess

import pytest

import pair_inputs
import pair_ref
from bam_layouts import BGZF_EOF, bgzf_pack
from test_pair_golden import BY_ID, CASES, DAMAGED, REFUSE, SAME, SUFFIXES, check_outputs, ids, input_path, read_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "highperformancengs_amd", "bin", "pick_pair")
TIMES = re.compile(r"at \d+\.\d{3} s")
ROUTE = re.compile(r"^\[hpn\] pick_pair: route (\w+);", re.M)
ROUTES = {0: "identity", 1: "join"}
OWN_INPUTS = pair_inputs.own_inputs()


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


# ---- the ABI ------------------------------------------------------------------------------------------------------

def feed(ctx, mate, data, cuts):
    a, n = 0, 0
    for c in cuts:
        info = ctx.fastq_pair_add(mate, data[a:c], last=(c == cuts[-1]))
        assert info.irregular == 0, info.irregular
        n += info.n_records
        a = c
    return n


def run_abi(ctx, a, b, cuts_a=None, cuts_b=None, interleaved=False, slice_bytes=1 << 24):
    """(result, the four outputs or None).  interleaved: the mates' chunks take turns."""
    cuts_a, cuts_b = cuts_a or [len(a)], cuts_b or [len(b)]
    ctx.fastq_pair_begin()
    if interleaved:
        pa = pb = na = nb = 0
        for k in range(max(len(cuts_a), len(cuts_b))):
            if k < len(cuts_a):
                na += ctx.fastq_pair_add(0, a[pa:cuts_a[k]], last=(k == len(cuts_a) - 1)).n_records
                pa = cuts_a[k]
            if k < len(cuts_b):
                nb += ctx.fastq_pair_add(1, b[pb:cuts_b[k]], last=(k == len(cuts_b) - 1)).n_records
                pb = cuts_b[k]
    else:
        nb = feed(ctx, 1, b, cuts_b)      # (READ2 first: any order)
        na = feed(ctx, 0, a, cuts_a)
    res = ctx.fastq_pair_finish()
    assert (res.n_records[0], res.n_records[1]) == (na, nb)
    if res.unverified:
        return res, None
    outs = [ctx.fastq_pair_output(w, slice_bytes) for w in range(4)]
    assert [len(o) for o in outs] == list(res.out_bytes)
    return res, outs


def check_abi(ctx, a, b, want_route=None, **kw):
    """The session against pair_ref: the route, the partition's counts and the four texts; where the certificate predicts the
    host, `unverified` with the certificate's failing record."""
    route, answer = pair_ref.device(a, b)
    if want_route is not None:
        assert route == want_route
    res, outs = run_abi(ctx, a, b, **kw)
    if route == "host":
        assert res.unverified == 1 and outs is None and (res.fail_mate, res.fail_record) == answer
        return res
    assert res.unverified == 0 and ROUTES[res.route] == route and res.fail_record == -1
    assert outs == pair_ref.outputs(a, b, answer)
    assert (res.n_pairs, res.n_single[0], res.n_single[1]) == (len(answer[0]), len(answer[1]), len(answer[3]))
    return res


OWN_PAIRS = sorted({n[:-5] for n in OWN_INPUTS})
REGULAR_PAIRS = [n for n in OWN_PAIRS if pair_ref.regular(OWN_INPUTS[n + "_a.fq"]) and pair_ref.regular(OWN_INPUTS[n + "_b.fq"])]


@pytest.mark.parametrize("name", REGULAR_PAIRS)
def test_abi_on_every_regular_input_pair(ctx, name):
    """Counts of 0, 1 and 2 per file and nA != nB, the space at every load border, B names shorter than k, gaps at the start and in
    the middle of both files, names without a space, high bytes, CRLF, a last line without its newline -- and the inputs on which
    no proposal verifies."""
    a, b = OWN_INPUTS[name + "_a.fq"], OWN_INPUTS[name + "_b.fq"]
    assert len(REGULAR_PAIRS) >= 45
    check_abi(ctx, a, b, want_route=BY_ID[name]["route"])


def test_abi_a_gap_of_5000_b_only_records(ctx):
    a, b = pair_inputs.big_gap(5000)
    res = check_abi(ctx, a, b, want_route="join")
    assert (res.n_pairs, res.n_single[0], res.n_single[1]) == (90, 0, 5000)


def test_abi_two_files_of_100000_records(ctx):
    a, b = pair_inputs.large(100000)
    res = check_abi(ctx, a, b, want_route="join", cuts_a=[len(a) // 3, len(a)], slice_bytes=1 << 20)
    assert res.n_records[0] > 97000 and res.n_single[0] > 1500 and res.n_single[1] > 1500
    # the same reads with nothing lost: the identity, and no comparison of the join's
    keys = list(range(0, 200000, 2))
    a, b = pair_inputs.mates(43, keys, keys, length=20)
    assert check_abi(ctx, a, b, want_route="identity").n_pairs == 100000


def test_abi_chunks_cut_at_every_byte(ctx):
    a, b = pair_inputs.mates(44, [1, 2, 4], [1, 3, 4])      # three records each
    assert a.count(b"\n") == b.count(b"\n") == 12 and pair_ref.device(a, b)[0] == "join"
    want = None
    for cut in range(len(a) + 1):
        res, outs = run_abi(ctx, a, b, cuts_a=[cut, len(a)], cuts_b=[min(cut, len(b)), len(b)], interleaved=bool(cut & 1))
        assert res.unverified == 0 and ROUTES[res.route] == "join"
        want = want or pair_ref.outputs(a, b, pair_ref.device(a, b)[1])
        assert outs == want, cut


def test_abi_one_byte_chunks_interleaved_and_one_mate_after_the_other(ctx):
    a, b = pair_inputs.mates(45, [1, 2, 4, 5, 7, 8, 9, 12], [1, 3, 4, 5, 9, 10, 12])
    ones = lambda d: list(range(1, len(d) + 1))
    for inter in (True, False):
        check_abi(ctx, a, b, want_route="join", cuts_a=ones(a), cuts_b=ones(b), interleaved=inter)


def test_abi_states_and_arguments(ctx):
    import highperformancengs_amd as hp
    a, b = OWN_INPUTS["same3_a.fq"], OWN_INPUTS["same3_b.fq"]
    ctx.fastq_pair_begin()
    ctx.fastq_pair_add(0, a, last=True)
    with pytest.raises(hp.HpnError):      # READ2 has not had its last chunk
        ctx.fastq_pair_finish()
    with pytest.raises(hp.HpnError):
        ctx.fastq_pair_add(2, b, last=True)
    with pytest.raises(hp.HpnError):      # READ1 is closed
        ctx.fastq_pair_add(0, a, last=True)
    ctx.fastq_pair_add(1, b, last=True)
    with pytest.raises(hp.HpnError):      # no output before finish
        ctx.fastq_pair_output(0)
    res = ctx.fastq_pair_finish()
    assert res.n_pairs == 3 and ROUTES[res.route] == "identity"
    with pytest.raises(hp.HpnError):
        ctx.fastq_pair_output(4)
    # irregular text closes the session
    ctx.fastq_pair_begin()
    assert ctx.fastq_pair_add(0, b"@a\nAC\n+\n", last=True).irregular != 0
    with pytest.raises(hp.HpnError):
        ctx.fastq_pair_add(1, b, last=True)
    # max_bytes counts both mates
    ctx.fastq_pair_begin(len(a) + 10)
    ctx.fastq_pair_add(0, a, last=True)
    with pytest.raises(hp.HpnError) as e:
        ctx.fastq_pair_add(1, b, last=True)
    assert e.value.status == hp._lib.E_CAPACITY


# ---- the tool -----------------------------------------------------------------------------------------------------

def run_tool(case, cwd, files=None):
    """Runs a manifest case in `cwd` with the inputs copied there under the names the recorder used (files: other bytes for them)."""
    os.makedirs(cwd)
    local = set()
    for a in case["args"]:
        if a in ("a.fq", "b.fq", "a.fq.gz", "b.fq.gz"):
            data = files[a[0]] if files else open(input_path(case[a[0]]), "rb").read()
            open(os.path.join(cwd, a), "wb").write(data)
            local.add(a)
    p = subprocess.run([TOOL] + case["args"], cwd=cwd, env={**os.environ, "HPN_TIMING": "1"}, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    return p, {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd) if fn not in local}


def check_same(case, p, got, what):
    err = p.stderr.decode("latin-1")
    assert p.returncode == 0 and p.stdout == b"", (what, err)
    route = ROUTE.findall(err)
    assert route == [case["route"]], (what, err)
    assert "".join(TIMES.sub("at T s", line) + "\n" for line in err.splitlines() if not line.startswith("[hpn]")) == case["stderr"], what
    check_outputs(case, {fn: gzip.decompress(data) for fn, data in got.items()})


@pytest.mark.parametrize("case", SAME, ids=ids(SAME))
def test_tool_matches_the_reference(case, tmp_path):
    p, got = run_tool(case, tmp_path / "r")
    check_same(case, p, got, "default")


@pytest.mark.parametrize("case", REFUSE + DAMAGED, ids=ids(REFUSE + DAMAGED))
def test_tool_refuses_where_the_reference_crashes(case, tmp_path):
    p, got = run_tool(case, tmp_path / "r")
    assert p.returncode == 2 and got == {} and p.stdout == b"", p.stderr
    assert b"pick_pair: " in p.stderr and not ROUTE.findall(p.stderr.decode("latin-1"))


@pytest.mark.parametrize("cid", ["thinned_300", "same3", "thinned_mispairs"])
def test_tool_input_routes(cid, tmp_path):
    """One case as plain text, one gzip member, several members and bgzip, the mates in different containers: the same outputs by
    the same route."""
    case = BY_ID[cid]
    a, b = read_input(case["a"]), read_input(case["b"])
    half = len(a) // 2
    forms = {"gzip": (gzip.compress(a), gzip.compress(b, 1)),
             "members": (gzip.compress(a[:half]) + gzip.compress(a[half:]), b),
             "bgzip": (bgzf_pack(a, 900) + BGZF_EOF, bgzf_pack(b, 65000) + BGZF_EOF),
             "mixed": (a, bgzf_pack(b, 300) + BGZF_EOF)}
    for what, (fa, fb) in forms.items():
        p, got = run_tool(case, tmp_path / what, {"a": fa, "b": fb})
        check_same(case, p, got, what)


def test_tool_input_that_is_no_regular_file_takes_the_host_walk(tmp_path):
    case = BY_ID["same3"]
    os.makedirs(tmp_path / "r")
    for side in ("a", "b"):
        open(tmp_path / "r" / (side + ".real"), "wb").write(read_input(case[side]))
    os.symlink("a.real", tmp_path / "r" / "a.fq")      # a link to a regular file is one
    os.mkfifo(tmp_path / "r" / "b.fq")
    writer = subprocess.Popen(["sh", "-c", "cat b.real > b.fq"], cwd=tmp_path / "r")
    p = subprocess.run([TOOL] + case["args"], cwd=tmp_path / "r", env={**os.environ, "HPN_TIMING": "1"}, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert writer.wait(timeout=60) == 0
    assert p.returncode == 0 and ROUTE.findall(p.stderr.decode("latin-1")) == ["host"], p.stderr
    check_outputs(case, {"o" + s: gzip.decompress(open(tmp_path / "r" / ("o" + s), "rb").read()) for s in SUFFIXES})


def test_every_recorded_case_is_run():
    assert len(SAME) + len(REFUSE) + len(DAMAGED) + 5 == len(CASES)
