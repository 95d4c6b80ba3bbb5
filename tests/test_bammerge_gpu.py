"""GPU: bam_merge on the device -- through the C ABI (hpn_bam_merge_*: the heap's keys and the HEAP_EMPTY check, the record store,
the running maximum inside every file, the sort over the ranked keys, the gather into merged order, cuts and CRC-32) and through
the tool -- against tests/bammerge_ref.py and the recorded runs of the compiled reference (tests/golden/bammerge/manifest.json).

Through the ABI every file's inflated stream is cut into batches by the test itself, as tests/test_bamsort_gpu.py does: BGZF
blocks are made that end exactly where a batch is to end, one hpn_bgzf_inflate_dev + hpn_bam_raw_index_dev +
hpn_bam_merge_add_raw_dev round per batch, the unfinished record (hpn_raw_info.tail_bytes) carried in front of the next.  A file
always ends on a batch's last record; files of no records lie between batches.  Through the tool every recorded case runs on the
device route and again with HPN_BAM_GPU=0; then the chain the tool exists for: bam_sort per part -> bam_merge -> bam_index ->
bam2depth."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bammerge_inputs
import bammerge_ref
import bamsort_ref
from bam_session import blocks_of_records, emit_all, every_boundary_and_inside, feed
from conftest import BIN, GOLDEN, HOOKS_BIN
from split_cases import stop_on_fault
from test_bammerge_golden import CASES, MANIFEST, check_run, lay_out

pytestmark = pytest.mark.gpu
TOOL = os.path.join(BIN, "bam_merge")
EMPTY = bammerge_ref.EMPTY


@pytest.fixture(scope="module")
def sets():
    s = bammerge_inputs.own_sets()
    assert bammerge_inputs.digests() == MANIFEST["inputs"]
    return s


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------------------

def run_tool(case, sets, work, env_extra, tool=TOOL):
    work.mkdir(parents=True)
    given = lay_out(case, sets, work)
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra)
    p = subprocess.run([tool] + case["args"], cwd=str(work), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    err = p.stderr.decode("latin-1")
    stop_on_fault(p.returncode, err)
    lines = err.splitlines(True)
    said = [ln for ln in lines if ln.startswith("[hpn]")]
    assert "".join(ln for ln in lines if not ln.startswith("[hpn]")) == case["stderr"], case["id"]
    check_run(case, p, work, given)
    return said


def early_exit(case):
    """usage, or an output that exists: the tool leaves before it chooses a route"""
    return len(case["args"]) - len(case["opts"]) < 3 or (case["old"] and "-f" not in case["opts"])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_tool_on_both_routes(case, sets, tmp_path):
    assert case["expect"] == "same"
    said = run_tool(case, sets, tmp_path / "dev", {"HPN_TIMING": "1"})
    kw = bammerge_ref.options(case["opts"])
    if early_exit(case):
        assert said == []
    elif case["route"] == "device":
        assert "[hpn] bam_merge: device route\n" in said, said
    elif kw.get("by_name") or kw.get("rg") or case["rc"] != 0:
        assert said == ["[hpn] bam_merge: host route\n"], said
    else:
        assert "[hpn] bam_merge: device route abandoned: host route\n" in said, said
        if case["set"] == "heap_empty_2p31m2":      # (a pos of -2 ends the device route earlier: the record index takes no pos below -1)
            assert any("(refID -1, pos 2147483646) is outside the device's domain (reason 1)" in ln for ln in said), said
    said = run_tool(case, sets, tmp_path / "host", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"})
    assert said == ([] if early_exit(case) else ["[hpn] bam_merge: host route\n"])
    if case["id"] in ("three_sorted", "unsorted_all", "heap_empty_mid", "no_eof"):          # without HPN_TIMING nothing but the reference's words
        assert run_tool(case, sets, tmp_path / "quiet", {}) == []


LAUNCHES = ["residues", "residues_u", "incompressible", "packed", "seventeen", "oversize", "unsorted_all"]


@pytest.mark.parametrize("cid", LAUNCHES)
def test_the_tool_with_one_small_chunk_a_launch(sets, tmp_path, cid):
    """the test-hooks build: chunks of 65,600 compressed bytes, one chunk a launch, with and without the read-ahead thread; slices
    of 1,000 records, so that the open block is carried (residues: 1,500 records)"""
    case = next(c for c in CASES if c["id"] == cid)
    for ahead in ("1", "0"):
        said = run_tool(case, sets, tmp_path / ahead, {"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1", "HPN_BAM_AHEAD": ahead, "HPN_TIMING": "1"},
                        tool=os.path.join(HOOKS_BIN, "bam_merge"))
        assert "[hpn] bam_merge: device route\n" in said, said
        (line,) = [ln for ln in said if " batches" in ln]
        assert int(line.split(" files")[0].split()[-1]) == len(sets[case["set"]]), line
        if cid == "incompressible":
            assert int(line.split(" batches")[0].split()[-1]) >= 3, line      # a file did fall into several ingest batches


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

def abi_merge(ctx, streams, cuts=(), slice_records=1 << 30, emit=True):
    """streams: per file the bytes of its records.  -> (BamMergeResult, order, blocks)"""
    import highperformancengs_amd as hp
    try:
        ctx.bam_merge_begin()
        for s in streams:
            ctx.bam_merge_next_file()
            info = feed(ctx, ctx.bam_merge_add_raw_dev, s, cuts)
            assert info is None or info.bad_record == -1
        res = ctx.bam_merge_finish()
        assert (res.n_files, res.bad_record, res.payload_bytes) == (len(streams), -1, sum(len(s) for s in streams))
        order = ctx.bam_merge_order(res.n_records)
        return res, order, emit_all(ctx, "merge", res.n_records, slice_records)[0] if emit else None
    except hp.HpnError as e:
        stop_on_fault(0, str(e))
        raise


def restated(recs):
    """recs: per file its records -> (session ordinals in the heap's order, the lifted count, the blocks)"""
    keys = [[bammerge_ref.key(r) for r in f] for f in recs]
    base = [sum(len(f) for f in recs[:k]) for k in range(len(recs))]
    order, lifted = bammerge_ref.effective_order(keys)
    assert order == bammerge_ref.heap_order(keys)
    return [base[f] + i for f, i in order], lifted, blocks_of_records([recs[f][i] for f, i in order])


@pytest.mark.parametrize("name", ["three_sorted", "unsorted_all", "pos_high", "empty_middle", "empty_first", "empty_last", "equal_keys"])
def test_abi_at_every_record_boundary_and_inside_records(ctx, sets, name):
    """every file in batches cut at every record boundary and inside every record: a file ends on its batch's last record, and a
    file of no records lies between two batches"""
    recs = [bammerge_ref.parse(f).recs[:25] for f in sets[name]]
    want_order, lifted, want = restated(recs)
    cuts = set().union(*[every_boundary_and_inside(f) for f in recs])
    for c in (cuts, set()):
        res, order, blocks = abi_merge(ctx, [b"".join(f) for f in recs], c)
        assert list(order) == want_order
        assert res.n_lifted == lifted and res.n_records == len(want_order)
        assert blocks == want


@pytest.mark.parametrize("name", ["residues", "oversize", "exact_fill", "seventeen", "all_empty"])
def test_emit_slices_carry_the_open_block(ctx, sets, name):
    """slices of 7, 1,000 and all records give the same blocks"""
    recs = [bammerge_ref.parse(f).recs for f in sets[name]]
    want_order, lifted, want = restated(recs)
    for per in (7, 1000, 1 << 30):
        res, order, blocks = abi_merge(ctx, [b"".join(f) for f in recs], set(range(50000, 10 ** 6, 50000)), per)
        assert list(order) == want_order and res.n_lifted == lifted
        assert blocks == want


def minimal(tid, pos, flag):
    """records of 37 bytes (an empty name's NUL and nothing else) from one array per field -> (n, 37) uint8, their keys"""
    n = len(tid)
    tid, pos, flag = np.asarray(tid, np.int32), np.asarray(pos, np.int32), np.asarray(flag, np.uint32)
    arr = np.zeros((n, 37), np.uint8)
    arr[:, 0:4] = np.frombuffer(struct.pack("<i", 33), np.uint8)
    arr[:, 4:8] = tid.view(np.uint8).reshape(n, 4)
    arr[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    arr[:, 12] = 1                                                        # l_read_name
    arr[:, 16:20] = (flag << 16).astype(np.uint32).view(np.uint8).reshape(n, 4)
    arr[:, 24:32] = 0xff                                                  # no mate
    keys = (tid.astype(np.int64).astype(np.uint64) << np.uint64(32)) | (((pos.astype(np.int64) + 1) << 1) & 0xffffffff).astype(np.uint64) | (flag >> 4).astype(np.uint64)
    return arr, keys


def random_file(rs, n, sorted_=False, n_tid=3):
    tid = rs.randint(-1, n_tid, n)
    pos = rs.randint(-1, 1 << 20, n)
    flag = 16 * rs.randint(0, 2, n)
    arr, keys = minimal(tid, pos, flag)
    if sorted_:
        o = np.argsort(keys, kind="stable")
        arr, keys = arr[o], keys[o]
    return arr, keys


def model(keys):
    """per-file key arrays -> (the order of a stable sort by the running maximum inside every file, the lifted count)"""
    eff = np.concatenate([np.maximum.accumulate(k) if len(k) else k for k in keys]) if keys else np.zeros(0, np.uint64)
    own = np.concatenate(keys) if keys else eff
    return np.argsort(eff, kind="stable"), int((eff != own).sum())


def merge_arrays(ctx, files, check_bytes=True, cuts=(1000003, 3000001)):
    """files: [(records (n, 37), keys)] -> BamMergeResult; the order and the lifted count are the model's, the payload the records
    in that order"""
    want, lifted = model([k for _, k in files])
    res, order, _ = abi_merge(ctx, [a.tobytes() for a, _ in files], set(cuts), emit=False)
    n = sum(len(a) for a, _ in files)
    assert res.n_records == n
    assert (order == want).all()
    assert res.n_lifted == lifted
    if check_bytes:
        info = ctx.bam_merge_emit(0, n, True)
        assert info.n_records == n
        assert ctx.bam_merge_payload() == np.concatenate([a for a, _ in files])[want].tobytes()
    return res


def number(files):
    """makes every record distinct: its session ordinal in the template length"""
    at = 0
    for a, _ in files:
        a[:, 32:36] = np.arange(at, at + len(a), dtype=np.uint32).view(np.uint8).reshape(len(a), 4)
        at += len(a)
    return files


@pytest.mark.parametrize("sizes", [(2047,), (2048,), (2049,), (2047, 2049), (2048, 2048, 5), (2048, 0, 1000), (1000, 1048, 3000), (700, 0, 0, 5000, 1)],
                         ids=lambda s: "_".join(map(str, s)))
def test_running_maximum_at_the_tile_seams(ctx, sizes):
    """unsorted files whose lengths put a file boundary one below, at and one above a tile of 2,048 records, at item 2,048 of the
    concatenation and in mid-tile; the heap agrees with the model where the restatement is quick"""
    rs = np.random.RandomState(sum(sizes))
    files = number([random_file(rs, n) for n in sizes])
    res = merge_arrays(ctx, files)
    assert res.n_lifted > 0
    if sum(sizes) < 5000:
        keys = [[int(x) for x in k] for _, k in files]
        base = np.cumsum([0] + [len(k) for k in keys])
        assert [int(base[f] + i) for f, i in bammerge_ref.heap_order(keys)] == list(model([k for _, k in files])[0])


def test_running_maximum_survives_65_tiles_and_stops_at_the_file(ctx):
    """one file of 133,121 minimal records whose FIRST record carries the largest key: every record behind it is lifted to it, across
    more than 64 tiles; the same records as two files cut at record 66,000: the second file does not inherit the first's maximum"""
    n = 133121
    rs = np.random.RandomState(23)
    arr, keys = random_file(rs, n, n_tid=300)
    top = int(np.argmax(keys))
    arr[[0, top]], keys[[0, top]] = arr[[top, 0]], keys[[top, 0]]
    assert keys[0] == keys.max() and (keys[1:] < keys[0]).sum() > n - 100
    one = number([(arr.copy(), keys.copy())])
    res = merge_arrays(ctx, one)
    assert res.n_lifted == int((keys != keys[0]).sum()) and res.n_lifted > n - 100
    assert (model([keys])[0] == np.arange(n)).all()                       # everything is lifted to one key: the file comes out as it is
    two = number([(arr[:66000].copy(), keys[:66000].copy()), (arr[66000:].copy(), keys[66000:].copy())])
    res = merge_arrays(ctx, two)
    second = np.maximum.accumulate(keys[66000:])
    assert res.n_lifted == int((keys[:66000] != keys[0]).sum()) + int((second != keys[66000:]).sum())
    assert second.max() < keys[0]                                         # ... and would be lifted further if the maximum leaked


def test_ties_keep_the_files_in_argument_order(ctx):
    """3 files x 3,000 records of ONE key come out file-major, as they went in; two sorted files whose few distinct keys interleave
    hold their order across the sort's tile seam at 8,192"""
    same = number([minimal(np.full(3000, 1), np.full(3000, 500), np.zeros(3000, np.uint32)) for _ in range(3)])
    res = merge_arrays(ctx, same)
    assert res.n_lifted == 0
    assert (model([k for _, k in same])[0] == np.arange(9000)).all()
    rs = np.random.RandomState(5)
    few = []
    for n in (6000, 7000):
        a, k = minimal(np.full(n, 1), np.sort(rs.randint(0, 4, n)), 16 * rs.randint(0, 2, n))
        o = np.argsort(k, kind="stable")
        few.append((a[o], k[o]))
    res = merge_arrays(ctx, number(few))
    assert res.n_lifted == 0 and res.n_records == 13000 > 8192


def test_the_rank_width_follows_the_targets(ctx):
    """the sort runs over the 32 bits of position and strand and the bits the ranks of the high words take, with refID -1 present
    and absent"""
    pos = 1 << 30                                                         # (pos + 1) << 1 has bit 31: the low word takes 32 bits
    for n in (1, 2, 3, 255, 256, 257):
        for unplaced in (True, False):
            tids = np.concatenate([np.arange(n), [-1] if unplaced else []]).astype(np.int64)
            half = len(tids) // 2
            files = number([minimal(tids[:half], np.full(half, pos), np.zeros(half, np.uint32)),
                            minimal(tids[half:], np.full(len(tids) - half, pos), np.zeros(len(tids) - half, np.uint32))])
            res = merge_arrays(ctx, files)
            top_rank = n - 1 + (1 if unplaced else 0)
            assert res.sort_bits == 32 + top_rank.bit_length(), (n, unplaced, res.sort_bits)


@pytest.mark.parametrize("file_at", [0, 2])
@pytest.mark.parametrize("later_batch", [False, True])
def test_abi_names_the_heap_empty_record(ctx, file_at, later_batch):
    """refID -1, reverse strand, pos 2^31 - 2: reason 1 and the session ordinal, in file 0 and in file 2, in the first batch of the
    file and in a later one.  (The other record with that key, pos -2, never comes this far: the record index refuses a pos below
    -1 as no record at all, and the tool's host route takes the job -- the recorded cases heap_empty_m2 and heap_empty_mid.)"""
    rs = np.random.RandomState(7)
    assert int(minimal([-1], [-2], [16])[1][0]) == EMPTY
    for pos in ((1 << 31) - 2,):
        files = [random_file(rs, 50) for _ in range(3)]
        at = 37 if later_batch else 3
        arr, _ = files[file_at]
        bad, key = minimal([-1], [pos], [16])
        assert int(key[0]) == EMPTY
        arr[at] = bad[0]
        ctx.bam_merge_begin()
        info = None
        for k, (a, _) in enumerate(files[:file_at + 1]):
            ctx.bam_merge_next_file()
            info = feed(ctx, ctx.bam_merge_add_raw_dev, a.tobytes(), {20 * 37, 30 * 37 + 5} if later_batch else set())
            assert (info.bad_record >= 0) == (k == file_at)
        ordinal = 50 * file_at + at
        assert (info.bad_record, info.bad_tid, info.bad_pos, info.reason) == (ordinal, -1, pos, 1)
        res = ctx.bam_merge_finish()
        assert (res.bad_record, res.bad_tid, res.bad_pos, res.reason) == (ordinal, -1, pos, 1)
        import highperformancengs_amd as hp
        with pytest.raises(hp.HpnError):
            ctx.bam_merge_emit(0, 1, True)           # nothing was merged


def test_abi_session_order_is_checked():
    import highperformancengs_amd as hp
    c = hp.Context(0)
    try:
        from highperformancengs_amd import _lib
        state = lambda e: e.value.status == _lib.E_STATE
        with pytest.raises(hp.HpnError) as e:
            c.bam_merge_add_raw_dev(None)            # before _begin
        assert state(e)
        with pytest.raises(hp.HpnError) as e:
            c.bam_merge_next_file()                  # before _begin
        assert state(e)
        c.bam_merge_begin()
        with pytest.raises(hp.HpnError) as e:
            c.bam_merge_add_raw_dev(None)            # before the first _next_file
        assert state(e)
        with pytest.raises(hp.HpnError) as e:
            c.bam_merge_emit(0, 1, True)             # before _finish
        assert state(e)
        c.bam_merge_next_file()
        arr, _ = minimal([0, 0], [5, 3], [0, 0])
        feed(c, c.bam_merge_add_raw_dev, arr.tobytes(), set())
        c.bam_merge_next_file()
        res = c.bam_merge_finish()
        assert (res.n_records, res.n_files, res.n_lifted, res.bad_record) == (2, 2, 1, -1)
        with pytest.raises(hp.HpnError) as e:
            c.bam_merge_next_file()                  # behind _finish
        assert state(e)
        with pytest.raises(hp.HpnError) as e:
            c.bam_merge_add_raw_dev(None)
        assert state(e)
        with pytest.raises(hp.HpnError):
            c.bam_merge_finish()
        with pytest.raises(hp.HpnError):
            c.bam_merge_emit(1, 1, True)             # not where the slice before ended
        c.bam_merge_begin()                          # a second _begin leaves nothing of the old session
        with pytest.raises(hp.HpnError):
            c.bam_merge_emit(0, 1, True)
        res = c.bam_merge_finish()
        assert (res.n_records, res.n_files, res.payload_bytes, res.n_lifted, res.sort_bits, res.bad_record) == (0, 0, 0, 0, 0, -1)
        info = c.bam_merge_emit(0, 5, True)
        assert (info.n_records, info.n_blocks, info.open_bytes) == (0, 0, 0)
        with pytest.raises(hp.HpnError):
            c.bam_merge_emit(0, 0, True)             # behind the call that ended the file
    finally:
        c.close()


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def run(tool, args, cwd, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra or {})
    p = subprocess.run([os.path.join(BIN, tool)] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
    return p


def test_sort_the_parts_then_merge_then_index_then_depth(tmp_path):
    """the committed rand.bam with its records shuffled and dealt into three files: bam_sort on each, bam_merge, bam_index,
    bam2depth -- against bam_sort on the whole shuffled file, bam_index, bam2depth: what bam2depth writes is byte-equal"""
    import bamsort_inputs
    data = open(os.path.join(GOLDEN, "bam", "rand.bam"), "rb").read()
    p = bamsort_ref.parse(data)
    assert len(p.recs) > 100
    recs = bamsort_inputs.shuffled(p.recs, 43)
    hdr = bamsort_ref.header_bytes(p.text.replace(b"SO:coordinate", b"SO:unsorted"), p.targets)
    bam = lambda rs: b"".join(bamsort_ref.member(b, 6) for b in bamsort_ref.cut(hdr, rs)) + bamsort_ref.EOF_BLOCK
    third = (len(recs) + 2) // 3
    outs = {}
    for which in ("parts", "whole"):
        d = tmp_path / which
        d.mkdir()
        if which == "parts":
            for k in range(3):
                (d / ("p%d.bam" % k)).write_bytes(bam(recs[k * third:(k + 1) * third]))
                q = run("bam_sort", ["p%d.bam" % k, "s%d" % k], d)
                assert q.returncode == 0, q.stderr.decode()
                os.remove(d / ("p%d.bam" % k))
            q = run("bam_merge", ["x.bam", "s0.bam", "s1.bam", "s2.bam"], d, {"HPN_TIMING": "1"})
            assert q.returncode == 0 and b"[hpn] bam_merge: device route\n" in q.stderr and b" 0 lifted" in q.stderr, q.stderr.decode()
            merged = bamsort_ref.parse((d / "x.bam").read_bytes())
            want, err, rc = bammerge_ref.merge([(d / ("s%d.bam" % k)).read_bytes() for k in range(3)], ["s0.bam", "s1.bam", "s2.bam"])
            assert (d / "x.bam").read_bytes() == want and rc == 0
            assert sorted(merged.recs) == sorted(p.recs)
            for k in range(3):
                os.remove(d / ("s%d.bam" % k))
        else:
            (d / "in.bam").write_bytes(bam(recs))
            q = run("bam_sort", ["in.bam", "x"], d)
            assert q.returncode == 0, q.stderr.decode()
            os.remove(d / "in.bam")
        q = run("bam_index", ["x.bam"], d, {"HPN_TIMING": "1"})
        assert q.returncode == 0 and b"[hpn] bam_index: device route\n" in q.stderr, q.stderr.decode()
        assert run("bam2depth", ["-w", "1000", "-o", "d", "x.bam"], d).returncode == 0
        made = sorted(fn for fn in os.listdir(d) if fn not in ("x.bam", "x.bam.bai"))
        assert any(fn.endswith(".bedGraph") for fn in made), made
        outs[which] = {fn: (d / fn).read_bytes() for fn in made}
    assert outs["parts"].keys() == outs["whole"].keys() and len(outs["parts"]) == 2      # the bedGraph and the depth file
    assert all(v for v in outs["parts"].values())
    assert outs["parts"] == outs["whole"]
