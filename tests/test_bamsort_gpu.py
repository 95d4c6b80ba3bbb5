"""GPU: bam_sort on the device -- through the C ABI (hpn_bam_sort_*: keys and checks, the record store, the sort over the ranked
keys, the gather into sorted order, cuts and CRC-32, stored framing) and through the tool -- against tests/bamsort_ref.py and the
recorded runs of the compiled reference (tests/golden/bamsort/manifest.json).

Through the ABI the inflated stream is cut into batches by the test itself, as tests/test_split_gpu.py does: BGZF blocks are made
that end exactly where a batch is to end, one hpn_bgzf_inflate_dev + hpn_bam_raw_index_dev + hpn_bam_sort_add_raw_dev round per
batch, the unfinished record (hpn_raw_info.tail_bytes) carried in front of the next.  Through the tool every recorded case runs
on the device route and again with HPN_BAM_GPU=0; then the chain the tool exists for: bam_sort -> bam_index -> bam2depth."""
import ctypes as C
import glob
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bai_ref
import bamsort_inputs
import bamsort_ref
from bam_session import emit_all, every_boundary_and_inside, expected_blocks, feed
from conftest import BIN, GOLDEN, HOOKS_BIN, in_hooks_build
from split_cases import stop_on_fault
from test_bamsort_golden import CASES, MANIFEST, check_bam

pytestmark = pytest.mark.gpu
FULL = bamsort_ref.FULL
TOOL = os.path.join(BIN, "bam_sort")


@pytest.fixture(scope="session")
def made(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bamsort_inputs_gpu"))
    assert bamsort_inputs.materialize(d) == MANIFEST["inputs"]
    return d


@pytest.fixture(scope="module")
def inputs():
    return bamsort_inputs.own_inputs()


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------------------

def run_tool(case, made, work, env_extra, tool=TOOL):
    work.mkdir(parents=True)
    if case["input"]:
        os.symlink(bamsort_inputs.path_of(case["input"], made), work / "in.bam")
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra)
    p = subprocess.run([tool] + case["args"], cwd=str(work), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    err = p.stderr.decode("latin-1")
    stop_on_fault(p.returncode, err)
    lines = err.splitlines(True)
    said = [ln for ln in lines if ln.startswith("[hpn]")]
    assert p.returncode == case["rc"], (case["id"], err[-2000:])
    assert "".join(ln for ln in lines if not ln.startswith("[hpn]")) == case["stderr"], case["id"]
    if case["out"] == "stdout":
        check_bam(case, p.stdout)
    else:
        assert p.stdout == b""
        out = work / case["out"] if case["out"] else None
        check_bam(case, out.read_bytes() if out is not None and out.exists() else None)
    assert sorted(fn for fn in os.listdir(work) if fn != "in.bam") == case["listing"], case["id"]      # no temporary file
    return said


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_tool_on_both_routes(case, made, tmp_path):
    assert case["expect"] == "same"
    said = run_tool(case, made, tmp_path / "dev", {"HPN_TIMING": "1"})
    if case["input"] and case["out"]:
        if "-n" in case["opts"]:
            assert "[hpn] bam_sort: host route\n" in said, said
        elif case["route"] == "device":
            assert "[hpn] bam_sort: device route\n" in said, said
        else:
            assert "[hpn] bam_sort: device route abandoned: host route\n" in said, said
    said = run_tool(case, made, tmp_path / "host", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"})
    if case["out"]:
        assert said == ["[hpn] bam_sort: host route\n"]
    if case["id"] in ("strands", "strands_m_3", "pos_out_m2", "no_eof"):          # without HPN_TIMING nothing but the reference's words
        assert run_tool(case, made, tmp_path / "quiet", {}) == []


LAUNCHES = ["eq_batches", "strands", "oversize", "residues", "packed_1000", "strands_l0", "strands_m_9", "oversize_l0"]


@pytest.mark.parametrize("cid", LAUNCHES)
def test_the_tool_with_one_small_chunk_a_launch(made, tmp_path, cid):
    """the test-hooks build: chunks of 65,600 compressed bytes, one chunk a launch, with and without the read-ahead thread; slices
    of 1,000 records, so that the open block is carried"""
    case = next(c for c in CASES if c["id"] == cid)
    for ahead in ("1", "0"):
        said = run_tool(case, made, tmp_path / ahead, {"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1", "HPN_BAM_AHEAD": ahead, "HPN_TIMING": "1"},
                        tool=os.path.join(HOOKS_BIN, "bam_sort"))
        assert "[hpn] bam_sort: device route\n" in said, said
        if cid == "eq_batches":
            (line,) = [ln for ln in said if "batches" in ln]
            assert int(line.split(" batches")[0].split()[-1]) >= 3, line      # equal keys did fall into different ingest batches


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

def abi_sort(ctx, recs, cuts, slice_records=1 << 30, stored=False):
    import highperformancengs_amd as hp
    try:
        ctx.bam_sort_begin()
        info = feed(ctx, ctx.bam_sort_add_raw_dev, b"".join(recs), cuts)
        assert info is None or info.bad_record == -1
        res = ctx.bam_sort_finish()
        assert (res.n_records, res.bad_record, res.payload_bytes) == (len(recs), -1, sum(len(r) for r in recs))
        order = ctx.bam_sort_order(res.n_records)
        sizes = ctx.bam_sort_sizes(res.n_records)
        blocks, image = emit_all(ctx, "sort", res.n_records, slice_records, stored)
        return res, order, sizes, blocks, image
    except hp.HpnError as e:
        stop_on_fault(0, str(e))
        raise


@pytest.mark.parametrize("name", ["tid_beyond", "targets_3", "unplaced_pos"])
def test_abi_at_every_record_boundary_and_inside_records(ctx, inputs, name):
    recs = bamsort_ref.parse(inputs[name]).recs[:40]
    want_order = np.argsort(bamsort_ref.model_keys(recs), kind="stable")
    want = expected_blocks(recs, want_order)
    for cuts in (every_boundary_and_inside(recs), set()):
        res, order, sizes, blocks, image = abi_sort(ctx, recs, cuts, stored=True)
        assert list(order) == list(want_order)
        assert list(sizes) == [len(r) for r in recs]
        assert blocks == want
        assert image == b"".join(bamsort_ref.member(p, 0) for p, _ in want)
        assert res.fresh_mem == bamsort_ref.fresh_mem([len(r) for r in recs])


@pytest.mark.parametrize("name", ["strands", "oversize", "exact_fill", "residues", "all_equal", "no_records"])
def test_emit_slices_carry_the_open_block(ctx, inputs, name):
    """slices of 1, 7 and all records give the same blocks"""
    recs = bamsort_ref.parse(inputs[name]).recs
    want_order = np.argsort(bamsort_ref.model_keys(recs), kind="stable") if recs else []
    want = expected_blocks(recs, want_order)
    for per in (1, 7, 1 << 30):
        if per == 1 and len(recs) > 600:
            continue
        res, order, sizes, blocks, _ = abi_sort(ctx, recs, set(range(50000, 10 ** 6, 50000)), per)
        assert list(order) == list(want_order)
        assert [(len(p), c) for p, c in blocks] == [(len(p), c) for p, c in want]
        assert blocks == want


def test_the_rank_width_follows_the_targets(ctx, inputs):
    """the sort runs over 32 bits of position and strand and the bits the ranks of the high words take"""
    for n, bits in ((1, 33), (2, 34), (3, 34), (255, 40), (256, 41), (257, 41)):
        recs = bamsort_ref.parse(inputs["targets_%d" % n]).recs
        tids = {bamsort_ref.fields(r)[0] for r in recs}
        assert {n - 1, 0, -1} <= tids
        res, order, _, _, _ = abi_sort(ctx, recs, set())
        assert list(order) == list(np.argsort(bamsort_ref.model_keys(recs), kind="stable"))
        assert res.sort_bits == bits, (n, res.sort_bits)


def test_abi_names_the_first_record_outside_the_domain(ctx, inputs):
    """(a pos below -1 never comes this far: the record index refuses it as no record at all)"""
    for name, reason in (("pos_out_2p30m1", 2), ("pos_out_2p31m1", 2)):
        recs = bamsort_ref.parse(inputs[name]).recs
        ordinal = next(i for i, r in enumerate(recs) if not bamsort_ref.POS_MIN <= bamsort_ref.fields(r)[1] <= bamsort_ref.POS_MAX)
        for cuts in (set(), every_boundary_and_inside(recs[:ordinal + 2])):
            ctx.bam_sort_begin()
            info = feed(ctx, ctx.bam_sort_add_raw_dev, b"".join(recs), cuts)
            tid, pos, _ = bamsort_ref.fields(recs[ordinal])
            assert (info.bad_record, info.bad_tid, info.bad_pos, info.reason) == (ordinal, tid, pos, reason)
            res = ctx.bam_sort_finish()
            assert (res.bad_record, res.reason) == (ordinal, reason)


def test_abi_session_order_is_checked(ctx):
    import highperformancengs_amd as hp
    ctx.bam_sort_begin()
    with pytest.raises(hp.HpnError):
        ctx.bam_sort_emit(0, 1, True)            # before _finish
    res = ctx.bam_sort_finish()
    assert (res.n_records, res.payload_bytes, res.bad_record) == (0, 0, -1)
    with pytest.raises(hp.HpnError):
        ctx.bam_sort_emit(1, 1, True)            # not where the slice before ended
    info = ctx.bam_sort_emit(0, 5, True)
    assert (info.n_records, info.n_blocks, info.open_bytes) == (0, 0, 0)
    with pytest.raises(hp.HpnError):
        ctx.bam_sort_emit(0, 0, True)            # behind the call that ended the file
    with pytest.raises(hp.HpnError):
        ctx.bam_sort_finish()


def plain_records(seed, n, lo, hi):
    """n records of lo .. hi bytes with keys over three targets and the unplaced, as one array per field"""
    rs = np.random.RandomState(seed)
    tid = rs.randint(-1, 3, n).astype(np.int32)
    pos = rs.randint(0, 1 << 20, n).astype(np.int32)
    flag = (16 * rs.randint(0, 2, n)).astype(np.uint32)
    size = rs.randint(lo, hi + 1, n)
    recs = []
    for k in range(n):
        body = struct.pack("<iiIIiiii", int(tid[k]), int(pos[k]), 1, int(flag[k]) << 16, 0, -1, -1, 0) + b"\0" + bytes(rs.randint(0, 256, size[k] - 37).astype(np.uint8))
        recs.append(struct.pack("<i", len(body)) + body)
    return recs


@pytest.mark.parametrize("hooks", [False, True])
def test_gather_writes_nothing_outside_its_records(request, ctx, hooks):
    """21,290 records of 37 .. 200 bytes emitted as slices of 9,000, 8,192 + 1 and 4,096 + 1 records -- a slice past a sort tile, a
    workgroup and (test-hooks build: 16 workgroups) the gather's grid seam.  The payload buffer keeps the size the first slice gave
    it: filled with a guard pattern before the later slices, it must hold the slice's bytes and the pattern behind them."""
    if hooks and in_hooks_build(request, {}):
        return
    recs = plain_records(31, 9000 + 8193 + 4097, 37, 200)
    order = np.argsort(bamsort_ref.model_keys(recs), kind="stable")
    out = [recs[i] for i in order]
    ctx.bam_sort_begin()
    feed(ctx, ctx.bam_sort_add_raw_dev, b"".join(recs), {400000, 1500000})
    res = ctx.bam_sort_finish()
    assert list(ctx.bam_sort_order(res.n_records)) == list(order)
    first, fill, room, model = 0, 0, None, bamsort_ref.cut(b"", out)
    seen = []
    for cnt in (9000, 8193, 4097):
        want = b"".join(out[first:first + cnt])
        if room is not None:
            assert fill + len(want) + 64 <= room
            guard = np.full(room, 0xA5, np.uint8)
            assert ctx.L.hpn_memcpy_h2d(ctx.h, C.c_void_p(where), guard.ctypes.data_as(C.c_void_p), room) == 0
            ctx.sync()
        info = ctx.bam_sort_emit(first, cnt, first + cnt == len(recs))
        before, (where, _) = None if room is None else where, ctx.bam_sort_payload_dev()
        assert before in (None, where)                                    # (the buffer has not moved)
        if room is None:
            room = fill + len(want)
        else:
            got = np.zeros(room, np.uint8)
            assert ctx.L.hpn_memcpy_d2h(ctx.h, got.ctypes.data_as(C.c_void_p), C.c_void_p(where), room) == 0
            ctx.sync()
            assert got[fill:fill + len(want)].tobytes() == want
            assert (got[fill + len(want):] == 0xA5).all()
        pay = ctx.bam_sort_payload()
        seen += [pay[b.off:b.off + b.len] for b in ctx.bam_sort_blocks(info.n_blocks)]
        first, fill = first + cnt, info.open_bytes
    assert seen == model


def test_sort_of_133121_records(ctx):
    """133,121 records of 37 bytes (an empty name's NUL and nothing else): a second look-back window of the scan within reach, keys
    over 300 targets and the unplaced; order, offsets and bytes against numpy"""
    n = 133121
    rs = np.random.RandomState(17)
    arr = np.zeros((n, 37), np.uint8)
    tid = rs.randint(-1, 300, n).astype(np.int32)
    pos = rs.randint(-1, 1 << 28, n).astype(np.int32)
    pos[rs.randint(0, n, 2000)] = 12345                                   # many equal keys
    flag = (16 * rs.randint(0, 2, n)).astype(np.uint32)
    arr[:, 0:4] = np.frombuffer(struct.pack("<i", 33), np.uint8)
    arr[:, 4:8] = tid.view(np.uint8).reshape(n, 4)
    arr[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    arr[:, 12] = 1                                                        # l_read_name
    arr[:, 16:20] = (flag << 16).astype(np.uint32).view(np.uint8).reshape(n, 4)
    arr[:, 24:32] = 0xff                                                  # no mate
    arr[:, 32:36] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)      # the template length: makes every record distinct
    keys = (tid.astype(np.int64).astype(np.uint64) << np.uint64(32)) | ((pos.astype(np.int64) + 1) << 1).astype(np.uint64) | (flag >> 4).astype(np.uint64)
    want = np.argsort(keys, kind="stable")
    ctx.bam_sort_begin()
    feed(ctx, ctx.bam_sort_add_raw_dev, arr.tobytes(), {1000003, 3000001})
    res = ctx.bam_sort_finish()
    assert (res.n_records, res.payload_bytes, res.bad_record) == (n, 37 * n, -1)
    assert res.sort_bits == 32 + 9                                         # 301 high words: 9 bits of rank
    assert (ctx.bam_sort_order(n) == want).all()
    info = ctx.bam_sort_emit(0, n, True)
    pay = ctx.bam_sort_payload()
    assert pay == arr[want].tobytes()
    bl = ctx.bam_sort_blocks(info.n_blocks)
    per = FULL // 37
    assert [b.len for b in bl] == [37 * per] * (n // per) + ([37 * (n % per)] if n % per else [])
    assert all(b.crc == zlib.crc32(pay[b.off:b.off + b.len]) & 0xffffffff for b in bl[::97])


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def run(tool, args, cwd, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra or {})
    p = subprocess.run([os.path.join(BIN, tool)] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
    return p


def test_sort_then_index_then_depth(tmp_path):
    """the committed rand.bam with its records shuffled: bam_sort, then bam_index, then bam2depth -- the file is the restatement's,
    the index samtools', the bedGraph that of the stable-sorted model file"""
    data = open(os.path.join(GOLDEN, "bam", "rand.bam"), "rb").read()
    p = bamsort_ref.parse(data)
    assert len(p.recs) > 100
    recs = bamsort_inputs.shuffled(p.recs, 41)
    hdr = bamsort_ref.header_bytes(p.text.replace(b"SO:coordinate", b"SO:unsorted"), p.targets)
    shuffled = b"".join(bamsort_ref.member(b, 6) for b in bamsort_ref.cut(hdr, recs)) + bamsort_ref.EOF_BLOCK
    model, _ = bamsort_ref.sort(shuffled)
    outs = {}
    for which in ("tool", "model"):
        d = tmp_path / which
        d.mkdir()
        if which == "tool":
            (d / "in.bam").write_bytes(shuffled)
            q = run("bam_sort", ["in.bam", "x"], d, {"HPN_TIMING": "1"})
            assert q.returncode == 0 and b"[hpn] bam_sort: device route\n" in q.stderr, q.stderr.decode()
            os.remove(d / "in.bam")
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
    assert hashlib.sha256(model).hexdigest() != hashlib.sha256(shuffled).hexdigest()
