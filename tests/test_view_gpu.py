"""GPU: bam_view on the device -- through the C ABI (hpn_bam_view_*: the keep bit, the line lengths and the domain checks, the record
store, the scans, order[], the SAM text slice by slice, the BAM slices with -Q's rescaled qualities, cuts and CRC-32) and through
the tool -- against tests/view_ref.py and the recorded runs of the compiled reference (tests/golden/view/manifest.json).

Through the ABI the file's inflated stream is cut into batches by the test itself, as tests/test_fixmate_gpu.py does.  Through the
tool every recorded case runs on the route the manifest names; `mixed` again with HPN_BAM_GPU=0; then the chains: bam_view -b -F
0x400 against bam_rmdup, bam_view -c against bam_sort's output."""
import os
import subprocess

import numpy as np
import pytest

import bamsort_ref
import fixmate_inputs
import rmdup_ref
import view_inputs
import view_ref
from bam_session import blocks_of_records, emit_all, every_boundary_and_inside, feed
from conftest import BIN, HOOKS_BIN
from split_cases import stop_on_fault
from test_view_golden import CASES, HOST_INPUTS, MANIFEST, run_case

pytestmark = pytest.mark.gpu
TOOL = os.path.join(BIN, "bam_view")
REASON = {"aux_float": 1, "aux_a_nul": 2, "name_nul_inside": 3, "aux_unknown": 4, "aux_b_negative": 4, "tid_beyond_header": 8, "mtid_beyond_header": 8}


@pytest.fixture(scope="module")
def inputs():
    assert view_inputs.digests() == MANIFEST["inputs"]
    return view_inputs.inputs()


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


def check_route(case, said):
    if case["expect"] == "refuse" and case["input"] not in REASON:
        return
    if not case["input"] and case["id"] not in ("missing_input", "missing_input_c"):
        assert said == [], said                    # the usage text: no route is chosen
    elif case["route"] == "device":
        assert "[hpn] bam_view: device route\n" in said, said
    elif case["route"] == "host" and case["expect"] == "same":
        assert said[0] == "[hpn] bam_view: host route\n", said
    else:
        assert "[hpn] bam_view: device route abandoned: host route\n" in said, said
        if case["input"] in REASON:
            assert any("is outside the device's domain (reason %d)" % REASON[case["input"]] in ln and "record " in ln for ln in said), said


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_tool_on_the_recorded_route(case, inputs, tmp_path):
    """output, stderr without [hpn] lines, status and what is left in the directory; the route HPN_TIMING names is the manifest's"""
    check_route(case, run_tool(case, inputs, tmp_path / "dev", {"HPN_TIMING": "1"}))
    if case["id"] in ("mixed_text", "mixed_b", "aux_float_text", "no_eof_h"):          # without HPN_TIMING nothing but the reference's words
        assert run_tool(case, inputs, tmp_path / "quiet", {}) == []


@pytest.mark.parametrize("cid", ["mixed_text", "mixed_fFqm", "mixed_fFqm_b", "mixed_h", "mixed_Q", "mixed_u", "mixed_s_b", "mixed_c"])
def test_the_host_route_writes_what_the_device_route_writes(inputs, tmp_path, cid):
    case = next(c for c in CASES if c["id"] == cid)
    assert run_tool(case, inputs, tmp_path / "host", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"})[:1] == ["[hpn] bam_view: host route\n"]


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["route"] == "device"])
def test_the_tool_with_one_small_chunk_a_launch(inputs, tmp_path, cid):
    """the test-hooks build: chunks of 65,600 compressed bytes, one chunk a launch, so that batches end inside runs of kept and
    dropped records and inside records; slices of 1,000 records, so that the open block and the text are carried over many slices"""
    case = next(c for c in CASES if c["id"] == cid)
    said = run_tool(case, inputs, tmp_path / "a", {"HPN_BAM_CHUNK": "65600", "HPN_BAM_ROUNDS": "1", "HPN_TIMING": "1"}, tool=os.path.join(HOOKS_BIN, "bam_view"))
    assert "[hpn] bam_view: device route\n" in said, said


def test_a_scale_beyond_int_is_the_same_on_both_routes(inputs, tmp_path):
    """-Q 2^30: the reference's int product overflows; here both routes multiply in 64 bits: 93 for every non-zero quality"""
    (tmp_path / "in.bam").write_bytes(inputs["lengths"])
    outs = []
    for env in ({"HPN_TIMING": "1"}, {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}):
        for args in (["-Q", "1073741824", "in.bam"], ["-Q", "1073741824", "-b", "-o", "o.bam", "in.bam"]):
            p = run("bam_view", args, tmp_path, env)
            assert p.returncode == 0
            outs.append(p.stdout if "-b" not in args else (tmp_path / "o.bam").read_bytes())
    assert outs[0] == outs[2] and outs[1] == outs[3]
    want, _, _, _ = view_ref.view(inputs["lengths"], ["-Q", "1073741824", "in.bam"])
    assert outs[0] == want and b"~~~" in want


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

def parsed(data):
    p = view_ref.parse(data)
    return p.recs, p.targets


RG_LIST = b"a2\nb1 zz\n"       # the -R file of the recorded cases


def groups_of(o, text):
    """(-R's IDs or None, the header's ID -> LB table behind drop_rg or None) of the options"""
    ids = set(RG_LIST.split()) if o.fn_rg is not None else None
    if ids is not None:
        text = view_ref.drop_rg(text, ids)
    return ids, (view_ref.rg_table(text) if o.library is not None else None)


def begin(ctx, emit, targets, args, text=b""):
    o = view_ref.options(args)
    ids, tbl = groups_of(o, text)
    ctx.bam_view_begin(emit, o.flag_on & 0xffffffff, o.flag_off & 0xffffffff, max(o.min_mapq, 0), o.min_qlen, o.qual_scale, o.frac > 0., o.seed,
                       view_ref.threshold(o.frac) if o.frac > 0. else 0, o.style, [nm for nm, _ in targets], rg_id=o.rg,
                       rg_ids=None if ids is None else sorted(ids), lib_ids=None if tbl is None else sorted(k for k, lb in tbl.items() if lb == o.library))
    return o


def kept_of(recs, o, text=b""):
    ids, tbl = groups_of(o, text)
    out = []
    for i, r in enumerate(recs):
        r = view_ref.scaled(r, o.qual_scale)
        if not view_ref.drops(o, r, ids, tbl):
            out.append((i, r))
    return out


def abi_text(ctx, recs, targets, args, cuts=(), slice_records=1 << 30, header=b""):
    import highperformancengs_amd as hp
    try:
        o = begin(ctx, ctx.VIEW_TEXT, targets, args, header)
        info = feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), cuts)
        assert info is None or info.bad_record == -1
        res = ctx.bam_view_finish()
        assert res.bad_record == -1 and res.n_records == len(recs)
        text, first = b"", 0
        while True:
            ti, piece = ctx.bam_view_text(first, slice_records)
            assert ti.n_records == min(slice_records, res.n_out - first) and ti.n_bytes == len(piece)
            text += piece
            first += ti.n_records
            if first >= res.n_out:
                break
        return o, res, list(ctx.bam_view_order(res.n_out)), text
    except hp.HpnError as e:
        stop_on_fault(0, str(e))
        raise


def check_text(ctx, recs, targets, args, cuts=(), slice_records=1 << 30, header=b""):
    o, res, order, text = abi_text(ctx, recs, targets, args, cuts, slice_records, header)
    kept = kept_of(recs, o, header)
    want = b"".join(view_ref.format_line(r, targets, o.style) + b"\n" for _, r in kept)
    assert order == [i for i, _ in kept] and res.n_out == len(kept) and res.text_bytes == len(want)
    assert text == want


def check_bam(ctx, recs, targets, args, cuts=(), slice_records=1 << 30, header=b""):
    import highperformancengs_amd as hp
    try:
        o = begin(ctx, ctx.VIEW_BAM, targets, args, header)
        info = feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), cuts)
        assert info is None or info.bad_record == -1
        res = ctx.bam_view_finish()
        kept = kept_of(recs, o, header)
        assert res.bad_record == -1 and res.n_out == len(kept) and res.payload_bytes == sum(len(r) for _, r in kept)
        assert list(ctx.bam_view_order(res.n_out)) == [i for i, _ in kept]
        blocks, image = emit_all(ctx, "view", res.n_out, slice_records, stored=True)
    except hp.HpnError as e:
        stop_on_fault(0, str(e))
        raise
    want = blocks_of_records([r for _, r in kept])
    assert [(len(p), c) for p, c in blocks] == [(len(p), c) for p, c in want]      # the CRC-32 saw the scaled bytes
    assert blocks == want
    assert image == b"".join(bamsort_ref.member(p, 0) for p, _ in want)


DEVICE_TEXT = sorted(c["input"] for c in CASES if c["id"].endswith("_text") and c["route"] == "device")      # (from the manifest: nothing is built at import)


@pytest.mark.parametrize("name", DEVICE_TEXT)
def test_abi_text_in_slices(ctx, inputs, name):
    """max_records 1, 7, 2,049 and all: the concatenation is the one-slice text and the restatement's"""
    recs, targets = parsed(inputs[name])
    big = len(recs) > 300
    for per in ((2049, 1 << 30) if big else (1, 7, 2049, 1 << 30)):
        check_text(ctx, recs, targets, ["-F", "0x400", "in.bam"], slice_records=per)
    if name in ("lengths", "numbers", "aux_all"):
        check_text(ctx, recs, targets, ["-X", "in.bam"], slice_records=7)
        check_text(ctx, recs, targets, ["-x", "-Q", "2", "in.bam"])
        check_text(ctx, recs[:40], targets, ["in.bam"], every_boundary_and_inside(recs[:40]), 1)


@pytest.mark.parametrize("name", ["lengths", "cuts_exact", "cuts_less", "cuts_more", "mixed", "runs", "last_only", "no_records"])
def test_abi_bam_slices_with_q(ctx, inputs, name):
    recs, targets = parsed(inputs[name])
    check_bam(ctx, recs, targets, ["-F", "0x400", "-Q", "2", "-b", "in.bam"])
    check_bam(ctx, recs, targets, ["-F", "0x400", "-Q", "2", "-b", "in.bam"], slice_records=7 if len(recs) < 300 else 2049)
    check_bam(ctx, recs, targets, ["-f", "0x400", "-b", "in.bam"], slice_records=1 if len(recs) < 300 else 1000)


def test_abi_filters_and_seams(ctx, inputs):
    """-f -F -q -m and -s together, batches cut inside runs and records"""
    recs, targets = parsed(inputs["mixed"])
    total = sum(len(r) for r in recs)
    check_text(ctx, recs, targets, ["-f", "0x1", "-F", "0x404", "-q", "20", "-m", "50", "in.bam"], {total // 3, total // 2 + 11, total - 50}, 1000)
    recs, targets = parsed(inputs["subsample"])
    for s in ("0.5", "7.25", "0.000001", "0.9999999", "1.0"):
        check_text(ctx, recs, targets, ["-s", s, "in.bam"], {len(recs[0]) + 3})
    recs, targets = parsed(inputs["runs"])
    at = sum(len(r) for r in recs[:view_inputs.SCAN_TILE - 1])
    check_text(ctx, recs, targets, ["-F", "0x400", "in.bam"], {at, at + 7, 2 * at}, 2049)


@pytest.mark.parametrize("name", ["rg", "rg_clean"])
def test_abi_read_groups(ctx, inputs, name):
    """-r, -R, -l and their combinations through the ABI: the walk to RG and the ID table, as text, BAM and count, batches cut
    inside records; on `rg` the table is the one a duplicated ID leaves (the last line wins)"""
    p = view_ref.parse(inputs[name])
    recs, targets = p.recs, p.targets
    total = sum(len(r) for r in recs)
    for args in (["-r", "a1"], ["-r", "nope"], ["-R", "list.txt"], ["-l", "libA"], ["-l", "libB"], ["-l", "nolib"], ["-r", "b1", "-l", "libA"],
                 ["-R", "list.txt", "-l", "libB"], ["-R", "list.txt", "-F", "0x400", "-q", "10"]):
        o = view_ref.options(args + ["in.bam"])
        assert len(kept_of(recs, o, p.text)) < len(recs)
        check_text(ctx, recs, targets, args + ["in.bam"], {total // 3 + 5, total // 2}, 7, header=p.text)
    check_bam(ctx, recs, targets, ["-R", "list.txt", "-l", "libA", "-b", "in.bam"], slice_records=7, header=p.text)
    o = begin(ctx, ctx.VIEW_COUNT, targets, ["-l", "libA", "-c", "in.bam"], p.text)
    feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), every_boundary_and_inside(recs[:20]))
    assert ctx.bam_view_finish().n_out == len(kept_of(recs, o, p.text))
    # an RG value without its end: the walk is needed, the record is outside the domain (5)
    bad = recs[:3] + [view_inputs.rec("open", 0, 5, "4M", 0, 30, "ACGT", [30] * 4, aux=b"RGZa1")]
    begin(ctx, ctx.VIEW_COUNT, targets, ["-r", "a1", "-c", "in.bam"], p.text)
    info = feed(ctx, ctx.bam_view_add_raw_dev, b"".join(bad), ())
    assert (info.bad_record, info.reason) == (3, view_ref.R_LAYOUT) == view_ref.device_reason(bad, 3, view_ref.options(["-r", "a1", "-c", "in.bam"]))
    assert ctx.bam_view_finish().bad_record == 3
    begin(ctx, ctx.VIEW_COUNT, targets, ["-c", "in.bam"], p.text)          # without the rule nothing walks there
    assert feed(ctx, ctx.bam_view_add_raw_dev, b"".join(bad), ()).bad_record == -1 and ctx.bam_view_finish().n_out == 4


def test_abi_counts(ctx, inputs):
    for name, args in (("mixed", ["-c", "-q", "30", "-f", "2"]), ("runs", ["-c", "-F", "0x400"]), ("aux_float", ["-c"]), ("no_records", ["-c"]), ("last_only", ["-c", "-F", "0x400"])):
        recs, targets = parsed(inputs[name])
        o = begin(ctx, ctx.VIEW_COUNT, targets, args + ["in.bam"])
        feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), ())
        res = ctx.bam_view_finish()
        assert (res.bad_record, res.n_out) == (-1, len(kept_of(recs, o))), name


def test_abi_names_the_first_record_outside_the_domain(ctx, inputs):
    import highperformancengs_amd as hp
    for name in sorted(REASON):
        recs, targets = parsed(inputs[name])
        o = begin(ctx, ctx.VIEW_TEXT, targets, ["in.bam"])
        bad, reason = view_ref.device_reason(recs, len(targets), o)
        assert reason == REASON[name]
        info = feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), {len(recs[0]) + 5})
        c = view_ref.core(recs[bad])
        assert (info.bad_record, info.bad_tid, info.bad_pos, info.reason) == (bad, c["tid"], c["pos"], reason), name
        res = ctx.bam_view_finish()
        assert (res.bad_record, res.reason, res.n_out) == (bad, reason, 0)
        with pytest.raises(hp.HpnError):
            ctx.bam_view_text(0, 1)


# ---- the chains ---------------------------------------------------------------------------------------------------------------------

def run(tool, args, cwd, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra or {})
    p = subprocess.run([os.path.join(BIN, tool)] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
    return p


def test_view_after_sort_and_against_rmdup(tmp_path):
    """pairs, every fourth one a duplicate of the pair before it and flagged 0x400 by the aligner's duplicate marker: bam_view -b -F
    0x400 keeps what bam_rmdup keeps, by construction; bam_view -c of bam_sort's output is the record count"""
    rs = np.random.RandomState(78)
    recs = []
    for k in range(400):
        if k % 4 != 3:
            tid, p1, gap = int(rs.randint(0, 3)), int(rs.randint(0, 200000)), int(rs.randint(40, 400))
        dup = 0x400 if k % 4 == 3 else 0
        b = fixmate_inputs.rec("c%d" % k, tid, p1 + gap, "50M", 0x93 | dup, l_seq=50, mtid=tid, mpos=p1, isize=-gap - 50)
        a = fixmate_inputs.rec("c%d" % k, tid, p1, "50M", 0x63 | dup, l_seq=50, mtid=tid, mpos=p1 + gap, isize=gap + 50)
        recs += [a, b]
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in fixmate_inputs.refs(3))
    aligned = fixmate_inputs.bam(recs, fixmate_inputs.header(fixmate_inputs.refs(3), text))
    sorted_model, _ = bamsort_ref.sort(aligned)
    d = tmp_path
    (d / "in.bam").write_bytes(aligned)
    q = run("bam_sort", ["in.bam", "s"], d, {"HPN_TIMING": "1"})
    assert q.returncode == 0 and (d / "s.bam").read_bytes() == sorted_model
    q = run("bam_view", ["-c", "s.bam"], d, {"HPN_TIMING": "1"})
    assert q.returncode == 0 and q.stdout == b"%d\n" % len(recs) and b"[hpn] bam_view: device route\n" in q.stderr, q.stderr.decode()
    q = run("bam_view", ["-b", "-F", "0x400", "-o", "v.bam", "s.bam"], d, {"HPN_TIMING": "1"})
    assert q.returncode == 0 and b"[hpn] bam_view: device route\n" in q.stderr, q.stderr.decode()
    q = run("bam_rmdup", ["s.bam", "x.bam"], d, {"HPN_TIMING": "1"})
    assert q.returncode == 0
    model, _, order = rmdup_ref.rmdup(sorted_model)
    assert (d / "x.bam").read_bytes() == model
    viewed = view_ref.parse((d / "v.bam").read_bytes()).recs
    assert len(viewed) == 600
    # rmdup keeps one pair of every duplicate set -- the flagged copy or the one before it -- at the same places
    key = lambda r: (view_ref.core(r)["tid"], view_ref.core(r)["pos"], view_ref.core(r)["flag"] & ~0x400)
    assert [key(r) for r in viewed] == [key(r) for r in view_ref.parse(model).recs]
