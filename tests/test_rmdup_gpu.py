"""GPU: bam_rmdup on the device -- through the C ABI (hpn_bam_rmdup_*: classes and checks, the record store, groups, name events,
placement, the gather of the survivors, cuts and CRC-32, stored framing) and through the tool -- against tests/rmdup_ref.py and
the recorded runs of the compiled reference (tests/golden/rmdup/manifest.json).

Through the ABI the inflated stream is cut into batches by the test itself, as tests/test_bamsort_gpu.py does: BGZF blocks are
made that end exactly where a batch is to end, one hpn_bgzf_inflate_dev + hpn_bam_raw_index_dev + hpn_bam_rmdup_add_raw_dev round
per batch, the unfinished record (hpn_raw_info.tail_bytes) carried in front of the next.  Through the tool every recorded case
runs on the device route and again with HPN_BAM_GPU=0; then the chain: bam_sort -> bam_rmdup -> bam_index -> bam2depth."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import bai_ref
import bamsort_inputs
import bamsort_ref
import rmdup_inputs
import rmdup_ref
from bam_session import emit_all, every_boundary_and_inside, expected_blocks, feed
from conftest import BIN, HOOKS_BIN
from split_cases import stop_on_fault
from test_rmdup_golden import CASES, MANIFEST, check_run

pytestmark = pytest.mark.gpu
TOOL = os.path.join(BIN, "bam_rmdup")


@pytest.fixture(scope="session")
def made(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rmdup_inputs_gpu"))
    assert rmdup_inputs.materialize(d) == MANIFEST["inputs"]
    return d


@pytest.fixture(scope="module")
def inputs():
    return rmdup_inputs.own_inputs()


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

class Model:
    """what rmdup_ref says of a file, with the libraries numbered as a caller of the ABI numbers them"""

    def __init__(self, data):
        p = bamsort_ref.parse(data)
        self.raw, self.n_ref = p.recs, len(p.targets)
        self.recs = [rmdup_ref.Rec(b) for b in p.recs]
        self.tbl = rmdup_ref.id_table(p.text)
        self.libs = [b"\t"] + sorted(set(self.tbl.values()))
        self.ids = sorted(self.tbl)
        self.lib_of_id = [self.libs.index(self.tbl[i]) for i in self.ids]

    def begin(self, ctx):
        ctx.bam_rmdup_begin(self.n_ref, self.ids, self.lib_of_id, len(self.libs))

    def plan(self):
        order, counts, unmatched, bad = rmdup_ref.plan(self.recs, self.tbl)
        libs = [(counts[l][1], counts[l][0], counts[l][2]) if l in counts else (0, 0, -1) for l in self.libs]
        present = {r.tid for r in self.recs}
        targets = [(t in present, unmatched.get(t, 0)) for t in range(self.n_ref)] + [(-1 in present, 0)]
        return order, libs, targets, bad


def abi_rmdup(ctx, model, cuts, slice_records=1 << 30, stored=False):
    import highperformancengs_amd as hp
    try:
        model.begin(ctx)
        info = feed(ctx, ctx.bam_rmdup_add_raw_dev, b"".join(model.raw), cuts)
        assert info is None or info.bad_record == -1, (info.bad_record, info.reason)
        res = ctx.bam_rmdup_finish()
        assert (res.n_records, res.bad_record) == (len(model.raw), -1), (res.bad_record, res.reason)
        order = ctx.bam_rmdup_order(res.n_out)
        libs, targets = ctx.bam_rmdup_counts()
        blocks, image = emit_all(ctx, "rmdup", res.n_out, slice_records, stored)
        return res, list(order), libs, targets, blocks, image
    except hp.HpnError as e:
        stop_on_fault(0, str(e))
        raise


def check_abi(ctx, model, cuts, slice_records=1 << 30, stored=False):
    want_order, want_libs, want_targets, bad = model.plan()
    assert bad is None
    res, order, libs, targets, blocks, image = abi_rmdup(ctx, model, cuts, slice_records, stored)
    assert order == want_order
    assert libs == want_libs
    assert targets == want_targets
    want = expected_blocks(model.raw, want_order)
    assert [(len(p), c) for p, c in blocks] == [(len(p), c) for p, c in want]
    assert blocks == want
    assert res.payload_bytes == sum(len(model.raw[i]) for i in want_order) and res.n_heads == sum(1 for r in model.recs if r.tid != -1 and rmdup_ref.classify(r) == "H")
    if stored:
        assert image == b"".join(bamsort_ref.member(p, 0) for p, _ in want)


@pytest.mark.parametrize("name", ["tails", "mixed"])
def test_abi_at_every_record_boundary_and_inside_records(ctx, inputs, name):
    """a 26-record file and the first 40 records of the general case (with its last five: the unplaced), cut at every record boundary
    and inside every record, and not at all"""
    model = Model(inputs[name])
    if len(model.raw) > 40:
        keep = model.raw[:35] + model.raw[-5:]
        model.raw, model.recs = keep, [rmdup_ref.Rec(b) for b in keep]
    for cuts in (every_boundary_and_inside(model.raw), set()):
        check_abi(ctx, model, cuts, stored=True)


@pytest.mark.parametrize("name", ["mixed", "qual_lengths", "groups", "interleaved", "batches", "names", "rg_places", "no_rg_lines", "residues", "oversize",
                                  "probe", "no_records"])
def test_abi_on_every_file_of_the_domain(ctx, inputs, name):
    """batches that end every 50,000 bytes and at chosen places inside groups; slices of 7 records and of all"""
    model = Model(inputs[name])
    sizes = np.cumsum([len(r) for r in model.raw]) if model.raw else np.zeros(0, np.int64)
    chosen = {int(sizes[k]) for k in (1, 2, 63, 64, 65, 299, 300) if k < len(sizes)} | set(range(50000, 10 ** 6, 50000))
    for per in (7, 1 << 30):
        check_abi(ctx, model, chosen, per)


def test_abi_names_the_first_record_outside_the_domain(ctx, inputs):
    files = {n: inputs[n] for n in ("rg_type_i", "aux_d", "first_unplaced", "only_unplaced", "pos_m1", "tid_returns", "inconsistent")}
    files["tid_beyond"] = rmdup_inputs.tid_beyond()
    for name, data in files.items():
        model = Model(data)
        first = rmdup_ref.first_refusal(model.recs, model.n_ref)
        if first is None:
            first = (model.plan()[3], rmdup_ref.R_INCONSISTENT)
        r = model.recs[first[0]]
        for cuts in (set(), every_boundary_and_inside(model.raw[:first[0] + 2])):
            model.begin(ctx)
            info = feed(ctx, ctx.bam_rmdup_add_raw_dev, b"".join(model.raw), cuts)
            res = ctx.bam_rmdup_finish()
            assert (res.bad_record, res.reason) == first, name
            assert (res.bad_tid, res.bad_pos) == ((-1, 0) if r.tid == -1 else (r.tid, r.pos)), name
            if first[1] != rmdup_ref.R_INCONSISTENT:
                assert (info.bad_record, info.reason) == first, name


def test_abi_session_order_is_checked(ctx):
    import highperformancengs_amd as hp
    ctx.bam_rmdup_begin(3)
    with pytest.raises(hp.HpnError):
        ctx.bam_rmdup_emit(0, 1, True)            # before _finish
    res = ctx.bam_rmdup_finish()
    assert (res.n_records, res.n_out, res.payload_bytes, res.bad_record) == (0, 0, 0, -1)
    with pytest.raises(hp.HpnError):
        ctx.bam_rmdup_emit(1, 1, True)            # not where the slice before ended
    info = ctx.bam_rmdup_emit(0, 5, True)
    assert (info.n_records, info.n_blocks, info.open_bytes) == (0, 0, 0)
    with pytest.raises(hp.HpnError):
        ctx.bam_rmdup_emit(0, 0, True)            # behind the call that ended the file
    with pytest.raises(hp.HpnError):
        ctx.bam_rmdup_finish()
    with pytest.raises(hp.HpnError):
        ctx.bam_rmdup_begin(3, [b"a"], [1], 1)    # a library beyond n_libs


def duplicated(seed, n_frag):
    """n_frag fragments over 2 targets, 1 .. 4 copies each, as sorted records"""
    rs = np.random.RandomState(seed)
    frags = [(int(rs.randint(0, 2)), int(rs.randint(0, 3000)) * 7, int(rs.randint(60, 200)), ["a", "b", None][int(rs.randint(0, 3))],
              [int(v) for v in rs.randint(10, 14, int(rs.randint(1, 5)))]) for _ in range(n_frag)]
    return rmdup_inputs.in_order(rmdup_inputs.pairs(frags, "d"))


def test_gather_writes_nothing_outside_its_records(ctx):
    """~15,000 records in, the ~6,000 survivors emitted as slices of 4,097, 1,025 and the rest.  The payload buffer keeps the size the first
    slice gave it: filled with a guard pattern before the later slices, it must hold the slice's bytes and the pattern behind them."""
    raw = duplicated(7, 3000)
    model = Model(rmdup_inputs.bgzf(rmdup_inputs.lay_sam(rmdup_inputs.H3, raw)))
    want_order, want_libs, _, _ = model.plan()
    out = [model.raw[i] for i in want_order]
    assert 4097 + 1025 + 100 < len(out) < len(raw) - 1000
    model.begin(ctx)
    feed(ctx, ctx.bam_rmdup_add_raw_dev, b"".join(model.raw), {400000, 900001})
    res = ctx.bam_rmdup_finish()
    assert res.n_out == len(out) and list(ctx.bam_rmdup_order(res.n_out)) == want_order and ctx.bam_rmdup_counts()[0] == want_libs
    first, fill, room, seen = 0, 0, None, []
    for cnt in (4097, 1025, len(out) - 4097 - 1025):
        want = b"".join(out[first:first + cnt])
        if room is not None:
            assert fill + len(want) + 64 <= room
            guard = np.full(room, 0xA5, np.uint8)
            assert ctx.L.hpn_memcpy_h2d(ctx.h, C.c_void_p(where), guard.ctypes.data_as(C.c_void_p), room) == 0
            ctx.sync()
        info = ctx.bam_rmdup_emit(first, cnt, first + cnt == len(out))
        before, (where, _) = None if room is None else where, ctx.bam_rmdup_payload_dev()
        assert before in (None, where)                                    # (the buffer has not moved)
        if room is None:
            room = fill + len(want)
        else:
            got = np.zeros(room, np.uint8)
            assert ctx.L.hpn_memcpy_d2h(ctx.h, got.ctypes.data_as(C.c_void_p), C.c_void_p(where), room) == 0
            ctx.sync()
            assert got[fill:fill + len(want)].tobytes() == want
            assert (got[fill + len(want):] == 0xA5).all()
        pay = ctx.bam_rmdup_payload()
        seen += [pay[b.off:b.off + b.len] for b in ctx.bam_rmdup_blocks(info.n_blocks)]
        first, fill = first + cnt, info.open_bytes
    assert seen == bamsort_ref.cut(b"", out)


# ---- the tool -----------------------------------------------------------------------------------------------------------------------

def run_tool(case, made, work, env_extra, tool=TOOL):
    work.mkdir(parents=True)
    if case["input"]:
        os.symlink(rmdup_inputs.path_of(case["input"], made), work / "in.bam")
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra)
    p = subprocess.run([tool] + case["args"], cwd=str(work), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    err = p.stderr.decode("latin-1")
    stop_on_fault(p.returncode, err)
    assert p.stdout == b""
    lines = err.splitlines(True)
    said = [ln for ln in lines if ln.startswith("[hpn]")]
    words = err if case["expect"] == "refuse" else "".join(ln for ln in lines if not ln.startswith("[hpn]"))
    out = work / case["out"] if case["out"] else None
    check_run(case, p.returncode, words, out.read_bytes() if out is not None and out.exists() else None, sorted(fn for fn in os.listdir(work) if fn != "in.bam"))
    return said


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_tool_on_both_routes(case, made, tmp_path):
    said = run_tool(case, made, tmp_path / "dev", {"HPN_TIMING": "1"})
    if case["input"] and case["out"]:
        if case["opts"]:
            assert "[hpn] bam_rmdup: host route\n" in said, said
        elif case["route"] == "device":
            assert "[hpn] bam_rmdup: device route\n" in said, said
        else:
            assert "[hpn] bam_rmdup: device route abandoned: host route\n" in said, said
    said = run_tool(case, made, tmp_path / "host", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"})
    if case["out"] and case["expect"] == "same":
        assert said == ["[hpn] bam_rmdup: host route\n"]
    if case["id"] in ("mixed", "tails", "inconsistent", "no_eof"):          # without HPN_TIMING nothing but the reference's words
        assert run_tool(case, made, tmp_path / "quiet", {}) == []


LAUNCHES = ["batches", "mixed", "groups", "oversize", "residues", "packed_1000"]


@pytest.mark.parametrize("cid", LAUNCHES)
def test_the_tool_with_one_small_chunk_a_launch(made, tmp_path, cid):
    """the test-hooks build: chunks of 65,600 compressed bytes, one chunk a launch, with and without the read-ahead thread; slices
    of 1,000 records, so that the open block is carried"""
    case = next(c for c in CASES if c["id"] == cid)
    for ahead in ("1", "0"):
        said = run_tool(case, made, tmp_path / ahead, {"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1", "HPN_BAM_AHEAD": ahead, "HPN_TIMING": "1"},
                        tool=os.path.join(HOOKS_BIN, "bam_rmdup"))
        assert "[hpn] bam_rmdup: device route\n" in said, said
        if cid == "batches":
            (line,) = [ln for ln in said if "batches" in ln]
            assert int(line.split(" batches")[0].split()[-1]) >= 3, line      # the group did fall into different ingest batches


def test_the_tool_refuses_what_the_reference_leaves_undefined(tmp_path):
    for name, data in (("stale", rmdup_inputs.unsorted_stale()), ("beyond", rmdup_inputs.tid_beyond())):
        work = tmp_path / name
        work.mkdir()
        (work / "in.bam").write_bytes(data)
        p = run("bam_rmdup", ["in.bam", "out.bam"], work, {"HPN_TIMING": "1"})
        err = p.stderr.decode()
        assert p.returncode == 2 and sorted(os.listdir(work)) == ["in.bam"], err
        assert "[hpn] bam_rmdup: device route abandoned: host route\n" in err and "the reference's behaviour is undefined here" in err


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def run(tool, args, cwd, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra or {})
    p = subprocess.run([os.path.join(BIN, tool)] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
    return p


def test_sort_then_rmdup_then_index_then_depth(tmp_path):
    """duplicated pairs shuffled: bam_sort, bam_rmdup, bam_index (its sortedness check passes), bam2depth -- every file is the
    restatement's, and the bedGraph is that of the restatement's file"""
    raw = duplicated(11, 400)
    hdr = rmdup_inputs.header(rmdup_inputs.refs(3), rmdup_inputs.text_with().replace("SO:coordinate", "SO:unsorted"))
    shuffled = b"".join(bamsort_ref.member(b, 6) for b in bamsort_ref.cut(hdr, bamsort_inputs.shuffled(raw, 41))) + bamsort_ref.EOF_BLOCK
    sorted_model, _ = bamsort_ref.sort(shuffled)
    model, words, order = rmdup_ref.rmdup(sorted_model)
    assert len(order) < len(raw) - 100
    outs = {}
    for which in ("tool", "model"):
        d = tmp_path / which
        d.mkdir()
        if which == "tool":
            (d / "in.bam").write_bytes(shuffled)
            q = run("bam_sort", ["in.bam", "s"], d, {"HPN_TIMING": "1"})
            assert q.returncode == 0 and b"[hpn] bam_sort: device route\n" in q.stderr, q.stderr.decode()
            assert (d / "s.bam").read_bytes() == sorted_model
            q = run("bam_rmdup", ["s.bam", "x.bam"], d, {"HPN_TIMING": "1"})
            err = q.stderr.decode()
            assert q.returncode == 0 and "[hpn] bam_rmdup: device route\n" in err, err
            assert "".join(ln for ln in err.splitlines(True) if not ln.startswith("[hpn]")) == words
            os.remove(d / "in.bam"), os.remove(d / "s.bam")
            assert (d / "x.bam").read_bytes() == model
        else:
            (d / "x.bam").write_bytes(model)
        q = run("bam_index", ["x.bam"], d, {"HPN_TIMING": "1"})
        assert q.returncode == 0 and b"[hpn] bam_index: device route\n" in q.stderr, q.stderr.decode()
        assert (d / "x.bam.bai").read_bytes() == bai_ref.index(model)[0]
        assert run("bam2depth", ["-w", "1000", "-o", "d", "x.bam"], d).returncode == 0
        (path,) = glob.glob(os.path.join(str(d), "*.bedGraph"))
        outs[which] = open(path, "rb").read()
    assert outs["tool"] and outs["tool"] == outs["model"]
