"""GPU: bamSplitChr on the device -- through the C ABI (hpn_bam_split_*: keys and checks, cuts, CRC-32, stored framing) and through
the tool -- against tests/split_ref.py and the recorded runs of the compiled reference (tests/golden/split/manifest.json).

Through the ABI the inflated stream is cut into batches by the test itself: BGZF blocks are made that end exactly where a batch is
to end, one block per hpn_bgzf_inflate_dev + hpn_bam_raw_index_dev + hpn_bam_split_add_raw_dev round, the unfinished record
(hpn_raw_info.tail_bytes) carried in front of the next -- at every record boundary and inside every record for the small inputs,
every 50,000 bytes (and as one batch) for the ones with cut edges.  What comes back per target -- the blocks' payloads and CRCs in
order, for level 0 the framed image -- must be what the restatement makes.  Through the tool every recorded case runs on the
device route; the cases with more than a chunk of compressed bytes run again with the test-hooks chunk size, one chunk a launch."""
import os
import zlib

import numpy as np
import pytest

import bam_layouts as BL
import split_cases as SC
import split_inputs
import split_ref
from conftest import HOOKS_BIN, in_hooks_build
from split_cases import CASES, MANIFEST

pytestmark = pytest.mark.gpu
FULL = split_ref.FULL


@pytest.fixture(scope="session")
def made(tmp_path_factory):
    return SC.materialize_checked(str(tmp_path_factory.mktemp("split_inputs")))


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def abi_split(ctx, bam, cuts, level0):
    import highperformancengs_amd as hp
    try:
        return _abi_split(ctx, bam, cuts, level0)
    except hp.HpnError as e:
        SC.stop_on_fault(0, str(e))
        raise


def _abi_split(ctx, bam, cuts, level0):
    """The records of `bam` (split_ref.Bam) through the session in batches that end at the stream offsets `cuts` (ascending,
    relative to the first record; the stream's end is added) -> (per target [(payload, crc)], level-0 image per target, counts,
    SplitInfo of the refusal or None)."""
    import torch
    stream = b"".join(r for _, _, r in bam.recs)
    cuts = sorted({c for c in cuts if 0 < c < len(stream)} | {len(stream)}) if stream else []
    n_ref = len(bam.names)
    blocks = [[] for _ in range(n_ref)]
    image = [b"" for _ in range(n_ref)]
    ctx.split_begin(n_ref, level0)

    def take(info):
        if info.bad_record >= 0:
            return info
        bl = ctx.split_blocks(info.n_blocks)
        assert len(bl) == info.n_blocks
        pay = ctx.split_payload()
        assert len(pay) == info.payload_bytes
        img = ctx.split_stored() if level0 else b""
        assert len(img) == info.stored_bytes == (sum(b.len + 31 for b in bl) if level0 else 0)
        at = 0
        for b in bl:
            assert 0 <= b.tid < n_ref and 0 < b.len <= FULL and b.off + b.len <= len(pay)
            blocks[b.tid].append((pay[b.off:b.off + b.len], b.crc))
            if level0:
                image[b.tid] += img[at:at + b.len + 31]
                at += b.len + 31
        if bl:
            assert (info.tid_first, info.tid_last) == (bl[0].tid, bl[-1].tid)
        return None

    front, at, bad = b"", 0, None
    for end in cuts:
        piece = stream[at:end]
        at = end
        members = [BL.bgzf_member(piece[i:i + 60000], 1) for i in range(0, len(piece), 60000)]      # (a batch of several blocks where it is long)
        table, comp, outo = np.zeros((len(members), 3), np.uint64), b"", len(front)
        for k, mem in enumerate(members):
            a, n, isz = BL.blocks(mem)[0]
            table[k] = (len(comp) + a, n | (isz << 32), outo)
            comp += mem
            outo += isz
        nb = len(members)
        d_comp = torch.from_numpy(np.frombuffer(comp + bytes(64), np.uint8).copy()).cuda()
        d_blocks = torch.from_numpy(table.view(np.int64)).cuda()
        d_out = torch.zeros(outo + 64, dtype=torch.uint8, device="cuda")
        if front:
            d_out[:len(front)] = torch.from_numpy(np.frombuffer(front, np.uint8).copy()).cuda()
        d_status = torch.zeros(nb, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.bgzf_inflate_dev(d_comp, d_blocks, nb, d_out, d_status)
        raw = ctx.bam_raw_index_dev(d_out, d_blocks, nb, 0, d_status)
        assert raw.flags & 3 == 0, raw.flags
        whole = front + piece
        front = whole[len(whole) - raw.tail_bytes:] if raw.tail_bytes else b""
        if raw.n_records:
            bad = take(ctx.split_add_raw_dev(d_out, False))
            if bad is not None:
                break
    if bad is None:
        assert front == b""
        bad = take(ctx.split_add_raw_dev(None, True))
    res, counts = ctx.split_finish(n_ref)
    return blocks, image, counts, bad


def expected(bam):
    """per target: [(payload, crc)] of the record blocks, and the level-0 image of them"""
    n_head = len(range(0, len(bam.header), FULL))
    want, image = [], []
    for pl, _ in split_ref.payloads(bam):
        want.append([(p, zlib.crc32(p) & 0xffffffff) for p in pl[n_head:]])
        image.append(b"".join(split_ref.member(p, 0) for p in pl[n_head:]))
    return want, image


def boundaries(bam):
    out, at = [], 0
    for _, _, r in bam.recs:
        at += len(r)
        out.append(at)
    return out


def every_boundary_and_inside(bam):
    """every record boundary, and inside every record: one byte in, inside the fixed fields, the middle, one byte from its end"""
    cuts, at = set(), 0
    for _, _, r in bam.recs:
        cuts |= {at + 1, at + 9, at + len(r) // 2, at + len(r) - 1, at + len(r)}
        at += len(r)
    return cuts


SMALL = ["opts", "empty_024", "only_unplaced", "one_each", "placed_unmapped", "colon_names", "plain2", "hdr_notext", "e", "wrap"]
LARGE = ["edges64", "edges", "oversize", "multiblock", "aligned", "t300", "rand", "layouts"]


@pytest.mark.parametrize("level0", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_abi_at_every_record_boundary_and_inside_records(ctx, made, name, level0):
    bam = split_ref.read(split_inputs.path_of(name, made))
    assert split_ref.first_offender(bam) is None
    want, wimg = expected(bam)
    for cuts in (every_boundary_and_inside(bam), set()):
        blocks, image, counts, bad = abi_split(ctx, bam, cuts, level0)
        assert bad is None
        assert blocks == want
        assert not level0 or image == wimg
        assert list(counts) == [sum(1 for t, _, _ in bam.recs if t == k) for k in range(len(bam.names))]


@pytest.mark.parametrize("level0", [False, True])
@pytest.mark.parametrize("name", LARGE)
def test_abi_cut_edges_across_batches(ctx, made, name, level0):
    """the open block carried from batch to batch: cuts every 50,000 bytes, at every record boundary (<= 64 batches), one batch"""
    bam = split_ref.read(split_inputs.path_of(name, made))
    assert split_ref.first_offender(bam) is None
    want, wimg = expected(bam)
    total = sum(len(r) for _, _, r in bam.recs)
    bounds = boundaries(bam)
    for cuts in (set(range(50000, total, 50000)), set(bounds[::max(1, len(bounds) // 64)]), set()):
        blocks, image, counts, bad = abi_split(ctx, bam, cuts, level0)
        assert bad is None
        assert [[(len(p), c) for p, c in t] for t in blocks] == [[(len(p), c) for p, c in t] for t in want]
        assert blocks == want
        assert not level0 or image == wimg
        assert list(counts) == [sum(1 for t, _, _ in bam.recs if t == k) for k in range(len(bam.names))]


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """70,000 records of 38 - 60 bytes over four targets (an empty one among them), a record of 70,000 bytes and one of exactly
    0xff00 among them and target changes far behind the first 4,096 records: one batch is 18 tiles of the block-count scan in
    the shipped library and 1,095 -- more than the 1,024 lanes of k_split_tiles -- in the test-hooks build"""
    from highperformancengs_amd import bamio
    rs = np.random.RandomState(77)
    sizes = rs.randint(42, 61, 70000)
    sizes[rs.randint(0, 70000, 9000)] = 38
    recs = [split_inputs.rec(rs, 0 if k < 30000 else 2 if k < 55000 else 3, 100 + k, int(s)) for k, s in enumerate(sizes)]
    recs[12345] = split_inputs.rec(rs, 0, 100 + 12345, 70000)
    recs[40000] = split_inputs.rec(rs, 2, 100 + 40000, FULL)
    recs += [split_inputs.rec(rs, -1, -1, 50) for _ in range(100)]
    path = str(tmp_path_factory.mktemp("many") / "many.bam")
    bamio.write_bam(path, split_inputs.refs(4), recs)
    bam = split_ref.read(path)
    assert len(bam.recs) == 70100 and split_ref.first_offender(bam) is None
    return bam, expected(bam)


@pytest.mark.parametrize("hooks", [False, True])
def test_abi_batches_of_many_tiles(request, ctx, many, hooks):
    """one batch of 70,100 records, and three: every tile's base from the scan of the tiles before it"""
    if hooks and in_hooks_build(request, {}):
        return
    bam, (want, wimg) = many
    total = sum(len(r) for _, _, r in bam.recs)
    for cuts in (set(), {total // 3, 2 * total // 3 + 11}):
        blocks, image, counts, bad = abi_split(ctx, bam, cuts, True)
        assert bad is None
        assert [[(len(p), c) for p, c in t] for t in blocks] == [[(len(p), c) for p, c in t] for t in want]
        assert blocks == want and image == wimg
        assert list(counts) == [30000, 0, 25000, 15000]


REFUSED = ["pos_back", "tid_back", "placed_after_unplaced", "pos_minus1", "pos_2p29", "tid_ge_nref"]


@pytest.mark.parametrize("name", REFUSED)
def test_abi_names_the_first_offending_record(ctx, made, name):
    """in one batch, at every record boundary (the offender is then a batch's first record: the state carried on the device) and
    inside the records"""
    bam = split_ref.read(split_inputs.path_of(name, made))
    ordinal, tid, pos, reason = split_ref.first_offender(bam)
    for cuts in (set(), set(boundaries(bam)), every_boundary_and_inside(bam)):
        _, _, _, bad = abi_split(ctx, bam, cuts, False)
        assert bad is not None and (bad.bad_record, bad.bad_tid, bad.bad_pos, bad.reason) == (ordinal, tid, pos, reason)


def test_abi_session_order_is_checked(ctx):
    import highperformancengs_amd as hp
    ctx.split_begin(2)
    ctx.split_add_raw_dev(None, True)
    with pytest.raises(hp.HpnError):
        ctx.split_add_raw_dev(None, True)        # behind the call that ended the file
    res, counts = ctx.split_finish(2)
    assert res.n_records == 0 and res.n_blocks == 0 and res.bad_record == -1 and list(counts) == [0, 0]
    with pytest.raises(hp.HpnError):
        ctx.split_finish(2)


def test_stored_framing_at_every_residue(ctx):
    """k_split_stored: payload starts at every residue mod 16 against every destination residue mod 16, lengths 1 .. 48 (+ lengths
    around the 16-byte pieces of a long block and a full one); a guard pattern around every block's image stays untouched"""
    import torch
    rs = np.random.RandomState(5)
    data = rs.randint(0, 256, 1 << 20).astype(np.uint8)
    d_data = torch.from_numpy(data).cuda()
    lengths = list(range(1, 49)) + [255, 256, 257, 4111, FULL - 1, FULL]
    spans, want, at = [], {}, 0
    for length in lengths:
        many = length <= 48
        for sr in (range(16) if many else (0, 5)):
            for dr in (range(16) if many else (0, 11)):
                src = 16 * (len(spans) * 7 % 60000) + sr
                at = (at + 40 + 15) // 16 * 16 + (dr - 23) % 16       # the payload lands at at + 23: residue dr
                payload = data[src:src + length].tobytes()
                crc = zlib.crc32(payload) & 0xffffffff
                spans.append((src, at, length, crc))
                want[at] = split_ref.member(payload, 0)
                assert len(want[at]) == length + 31
                at += length + 31
    guard = np.full(at + 64, 0xA5, np.uint8)
    d_img = torch.from_numpy(guard.copy()).cuda()
    ctx.bgzf_stored_dev(d_data, spans, d_img)
    got = d_img.cpu().numpy()
    expect = guard.copy()
    for o, m in want.items():
        expect[o:o + len(m)] = np.frombuffer(m, np.uint8)
    assert {((s[0]) % 16, (s[1] + 23) % 16) for s in spans if s[2] <= 48} == {(a, b) for a in range(16) for b in range(16)}
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, bad[:8]


# ---- the tool -----------------------------------------------------------------------------------------------------------------------

ON_DEVICE = ["d_edges64", "u_edges64", "1_edges64", "d_multiblock", "d_repack97", "d_repack20000", "u_rand", "d_layouts", "two_inputs_u"]


@pytest.mark.parametrize("cid", [c["id"] for c in MANIFEST["cases"]])
def test_the_tool_on_the_device_route(made, tmp_path, cid):
    SC.check_tool(CASES[cid], made, tmp_path, {"HPN_TIMING": "1"})
    if cid in ON_DEVICE:
        assert any("GPU split" in ln and "abandoned" not in ln for ln in SC.HPN_LINES), SC.HPN_LINES


@pytest.mark.parametrize("opt", [[], ["-u", "x"]])
def test_the_tool_on_300_targets(made, tmp_path, opt):
    """one output file open at a time: 300 files of 0 - 2 records, against the restatement"""
    SC.check_tool(SC.model_case("t300", "t300", opt + ["-o", "o", "in.bam"], made), made, tmp_path, {"HPN_TIMING": "1"})
    assert any("GPU split" in ln and "abandoned" not in ln for ln in SC.HPN_LINES), SC.HPN_LINES


CHUNKED = [c["id"] for c in MANIFEST["cases"] if c["expect"] == "same" and c["inputs"] and
           c["inputs"][0] in ("edges64", "edges", "oversize", "multiblock", "aligned", "repack97", "repack20000")]


@pytest.mark.parametrize("cid", CHUNKED)
def test_the_tool_with_one_small_chunk_a_launch(made, tmp_path, cid):
    """the test-hooks build: chunks of 65,600 compressed bytes, one chunk a launch, with and without the read-ahead thread"""
    for ahead in ("1", "0"):
        work = tmp_path / ahead
        work.mkdir()
        SC.check_tool(CASES[cid], made, work, {"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1", "HPN_BAM_AHEAD": ahead, "HPN_TIMING": "1"},
                      tool=os.path.join(HOOKS_BIN, "bamSplitChr"))
    if cid.endswith("edges64") or cid.endswith("multiblock"):
        assert any("GPU split" in ln and "abandoned" not in ln for ln in SC.HPN_LINES), SC.HPN_LINES


def test_pos_going_backwards_across_a_batch_cut(ctx, tmp_path):
    """a file of two chunks whose second chunk's first record lies behind the first chunk's last: through the ABI (the carried
    state) and through the hooks tool with one chunk a launch"""
    import subprocess
    from highperformancengs_amd import bamio
    rs = np.random.RandomState(9)
    recs = [split_inputs.rec(rs, 0, 100 + k, 3000) for k in range(160)]      # (~310 KB compressed: five chunks)
    recs[40].pos = 5
    path = str(tmp_path / "in.bam")
    bamio.write_bam(path, split_inputs.refs(1), recs)
    bam = split_ref.read(path)
    assert split_ref.first_offender(bam)[:2] == (40, 0)
    _, _, _, bad = abi_split(ctx, bam, {40 * 3000}, False)
    assert (bad.bad_record, bad.bad_pos, bad.reason) == (40, 5, 4)
    assert os.path.getsize(path) > 2 * 65600
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update({"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1"})
    p = subprocess.run([os.path.join(HOOKS_BIN, "bamSplitChr"), "-o", "o", "in.bam"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 2 and "record 40 (refID 0, pos 5)" in p.stderr.decode()
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam", "in.bam.bai"]
