"""GPU: bam_fixmate on the device -- through the C ABI (hpn_bam_fixmate_*: classes, alignment ends and the domain checks, the record
store, names compared with the live record in front, runs, roles, the write counts' scan, order[] and the patches, the gather,
the rewritten core fields and the CT field, cuts and CRC-32) and through the tool -- against tests/fixmate_ref.py and the
recorded runs of the compiled reference (tests/golden/fixmate/manifest.json).

Through the ABI the file's inflated stream is cut into batches by the test itself, as tests/test_rmdup_gpu.py does: BGZF blocks
are made that end exactly where a batch is to end, one hpn_bgzf_inflate_dev + hpn_bam_raw_index_dev +
hpn_bam_fixmate_add_raw_dev round per batch, the unfinished record (hpn_raw_info.tail_bytes) carried in front of the next -- so a
pending record and its mate lie in different batches, with skipped records on both sides of the seam.  Through the tool every
recorded case runs on the device route and again with HPN_BAM_GPU=0; then the chain the tool exists for: bam_fixmate -> bam_sort
-> bam_rmdup -> bam_index."""
import os
import subprocess

import numpy as np
import pytest

import bai_ref
import bamsort_ref
import fixmate_inputs
import fixmate_ref
import rmdup_ref
from bam_session import blocks_of_records, emit_all, every_boundary_and_inside, feed
from conftest import BIN, HOOKS_BIN
from split_cases import stop_on_fault
from test_fixmate_golden import CASES, MANIFEST, run_case

pytestmark = pytest.mark.gpu
TOOL = os.path.join(BIN, "bam_fixmate")


@pytest.fixture(scope="module")
def inputs():
    f = fixmate_inputs.own_inputs()
    assert fixmate_inputs.digests() == MANIFEST["inputs"]
    return f


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------------------

def run_tool(case, inputs, work, env_extra, tool=TOOL):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra)
    err = run_case(tool, case, inputs, work, env, on_exit=stop_on_fault)
    return [ln for ln in err.splitlines(True) if ln.startswith("[hpn]")]


def chooses_a_route(case):
    return len([a for a in case["args"] if a != "-r"]) >= 2


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_tool_on_both_routes(case, inputs, tmp_path):
    said = run_tool(case, inputs, tmp_path / "dev", {"HPN_TIMING": "1"})
    if not chooses_a_route(case):
        assert said == []
    elif case["route"] == "device":
        assert "[hpn] bam_fixmate: device route\n" in said, said
    elif case["stdin"] or case["out"] == "stdout" or case["id"] == "missing_input":
        assert said[0] == "[hpn] bam_fixmate: host route\n", said
    else:
        assert "[hpn] bam_fixmate: device route abandoned: host route\n" in said, said
        reason = {"op_back": 1, "op_ten": 1, "op_ten_not_carried": 1, "op_eleven_carried": 1, "name_nul_inside": 2, "tid_beyond_header": 3}[case["input"]]
        assert any("is outside the device's domain (reason %d)" % reason in ln for ln in said), said
    said = run_tool(case, inputs, tmp_path / "host", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"})
    assert said[:1] == (["[hpn] bam_fixmate: host route\n"] if chooses_a_route(case) else [])
    if case["id"] in ("mixed", "mixed_r", "no_eof", "op_back"):          # without HPN_TIMING nothing but the reference's words
        assert run_tool(case, inputs, tmp_path / "quiet", {}) == []


@pytest.mark.parametrize("cid", ["mixed", "mixed_r", "slice_between_halves", "ct_straddles_cut", "grown_past_block", "ct_text", "run_past_tile"])
def test_the_tool_with_one_small_chunk_a_launch(inputs, tmp_path, cid):
    """the test-hooks build: chunks of 65,600 compressed bytes, one chunk a launch; slices of 1,000 records, so that the open block
    is carried from slice to slice and a slice ends between a pair's halves (slice_between_halves)"""
    case = next(c for c in CASES if c["id"] == cid)
    said = run_tool(case, inputs, tmp_path / "a", {"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1", "HPN_TIMING": "1"}, tool=os.path.join(HOOKS_BIN, "bam_fixmate"))
    assert "[hpn] bam_fixmate: device route\n" in said, said


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

def abi_fixmate(ctx, recs, target_len, remove, cuts=(), slice_records=1 << 30):
    """-> (FixmateResult, order, blocks)"""
    import highperformancengs_amd as hp
    try:
        ctx.bam_fixmate_begin(remove, target_len)
        info = feed(ctx, ctx.bam_fixmate_add_raw_dev, b"".join(recs), cuts)
        assert info is None or info.bad_record == -1
        res = ctx.bam_fixmate_finish()
        assert res.bad_record == -1 and res.n_records == len(recs)
        order = ctx.bam_fixmate_order(res.n_out)
        return res, list(order), emit_all(ctx, "fixmate", res.n_out, slice_records)[0]
    except hp.HpnError as e:
        stop_on_fault(0, str(e))
        raise


def restated(recs, target_len, remove):
    out, n = fixmate_ref.machine(recs, target_len, remove)
    return [i for i, _ in out], n, blocks_of_records([r for _, r in out]), sum(len(r) for _, r in out)


def check_abi(ctx, recs, target_len, remove, cuts=(), slice_records=1 << 30):
    want_order, n, want, payload = restated(recs, target_len, remove)
    res, order, blocks = abi_fixmate(ctx, recs, target_len, remove, cuts, slice_records)
    assert order == want_order
    assert (res.n_out, res.n_pairs, res.n_singletons, res.n_tags, res.bytes_added, res.payload_bytes) == (
        len(want_order), n["pairs"], n["singletons"], n["tags"], n["added"], payload)
    assert [(len(p), c) for p, c in blocks] == [(len(p), c) for p, c in want]      # the CRC-32 saw the patched bytes
    assert blocks == want


def parsed(data):
    p = fixmate_ref.parse(data)
    return p.recs, [ln for _, ln in p.targets]


DEVICE = sorted(n for n in fixmate_inputs.names() if fixmate_ref.route(fixmate_inputs.own_inputs()[n]) == "device")


@pytest.mark.parametrize("remove", [False, True], ids=["keep", "r"])
@pytest.mark.parametrize("name", ["skipped_between", "run_lengths", "ends_pending", "flags_and_ends", "only_skipped"])
def test_abi_at_every_record_boundary_and_inside_records(ctx, inputs, name, remove):
    """batches cut at every record boundary and inside every record: the pending record in one batch and its mate in the next, with
    skipped records on both sides of the seam"""
    recs, tl = parsed(inputs[name])
    check_abi(ctx, recs[:40], tl, remove, every_boundary_and_inside(recs[:40]))


@pytest.mark.parametrize("name", DEVICE)
def test_abi_on_every_file_of_the_domain(ctx, inputs, name):
    """one batch, one slice and slices of 7 and of 1,000 records, with and without -r"""
    recs, tl = parsed(inputs[name])
    check_abi(ctx, recs, tl, False)
    check_abi(ctx, recs, tl, True, slice_records=1000 if len(recs) > 500 else 7)
    if name in ("mixed", "ct_straddles_cut"):
        total = sum(len(r) for r in recs)
        check_abi(ctx, recs, tl, False, cuts={total // 3, total // 2, total - 50}, slice_records=7)


def test_the_parity_crosses_the_scans_tile(ctx, inputs):
    """a run of equal names one longer than the scan's tile: 1,024 pairs and a singleton in front of the next name"""
    recs, tl = parsed(inputs["run_past_tile"])
    want_order, n, _, _ = restated(recs, tl, False)
    assert n["pairs"] == fixmate_inputs.SCAN_TILE // 2 + 1 and n["singletons"] == 2
    check_abi(ctx, recs, tl, False, slice_records=1000)


def test_abi_names_the_first_record_outside_the_domain(ctx, inputs):
    import highperformancengs_amd as hp
    for name, cuts in (("op_back", ()), ("op_ten", ()), ("op_eleven_carried", ()), ("name_nul_inside", ()), ("tid_beyond_header", ()), ("op_ten_not_carried", {100})):
        recs, tl = parsed(inputs[name])
        bad, reason = fixmate_ref.device_reason(recs, len(tl))
        ctx.bam_fixmate_begin(False, tl)
        info = feed(ctx, ctx.bam_fixmate_add_raw_dev, b"".join(recs), cuts)
        c = fixmate_ref.core(recs[bad])
        assert (info.bad_record, info.bad_tid, info.bad_pos, info.reason) == (bad, c["tid"], c["pos"], reason), name
        res = ctx.bam_fixmate_finish()
        assert (res.bad_record, res.reason, res.n_out) == (bad, reason, 0)
        with pytest.raises(hp.HpnError):
            ctx.bam_fixmate_emit(0, 1, True)


def test_abi_session_order_is_checked(ctx, inputs):
    import highperformancengs_amd as hp
    recs, tl = parsed(inputs["ends_pair"])
    ctx.bam_fixmate_begin(False, tl)
    with pytest.raises(hp.HpnError):
        ctx.bam_fixmate_emit(0, 1, True)          # before _finish
    feed(ctx, ctx.bam_fixmate_add_raw_dev, b"".join(recs), ())
    res = ctx.bam_fixmate_finish()
    with pytest.raises(hp.HpnError):
        ctx.bam_fixmate_finish()                  # twice
    with pytest.raises(hp.HpnError):
        ctx.bam_fixmate_emit(1, 1, False)         # not the next slice
    assert len(emit_all(ctx, "fixmate", res.n_out, 2)[0]) == 1
    image = ctx.bam_fixmate_stored()              # the last slice's blocks framed for level 0
    want = b"".join(bamsort_ref.member(p, 0) for p in bamsort_ref.cut(b"", [r for _, r in fixmate_ref.machine(recs, tl, False)[0]]))
    assert image == want


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def run(tool, args, cwd, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra or {})
    p = subprocess.run([os.path.join(BIN, tool)] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
    return p


def test_fixmate_then_sort_then_rmdup_then_index(tmp_path):
    """aligner output -- name-adjacent pairs with unfilled mate fields, every fourth pair a duplicate of the one before it -- through
    bam_fixmate, bam_sort, bam_rmdup and bam_index on the device: every file is the restatement's, and rmdup, which reads the
    mate fields fixmate filled, finds the duplicates"""
    rs = np.random.RandomState(77)
    recs = []
    for k in range(400):
        if k % 4 != 3:
            tid, p1, gap = int(rs.randint(0, 3)), int(rs.randint(0, 200000)), int(rs.randint(40, 400))
        recs += fixmate_inputs.pair("c%d" % k, tid, p1, p1 + gap, "50M", "50M", 0x63, 0x93, l_seq=50)
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in fixmate_inputs.refs(3))
    aligned = fixmate_inputs.bam(recs, fixmate_inputs.header(fixmate_inputs.refs(3), text))
    fixed, _, rc = fixmate_ref.fixmate(aligned)
    assert rc == 0
    sorted_model, _ = bamsort_ref.sort(fixed)
    model, words, order = rmdup_ref.rmdup(sorted_model)
    assert len(order) <= len(recs) - 150          # the duplicates went
    unfixed, _, _ = rmdup_ref.rmdup(bamsort_ref.sort(aligned)[0])
    assert unfixed != model                       # without fixmate rmdup acts on unfilled mate fields
    d = tmp_path
    (d / "in.bam").write_bytes(aligned)
    for tool, args, out, want in (("bam_fixmate", ["in.bam", "f.bam"], "f.bam", fixed), ("bam_sort", ["f.bam", "s"], "s.bam", sorted_model),
                                  ("bam_rmdup", ["s.bam", "x.bam"], "x.bam", model), ("bam_index", ["x.bam"], "x.bam.bai", bai_ref.index(model)[0])):
        q = run(tool, args, d, {"HPN_TIMING": "1"})
        assert q.returncode == 0 and ("[hpn] %s: device route\n" % tool).encode() in q.stderr, q.stderr.decode()
        assert (d / out).read_bytes() == want, tool
