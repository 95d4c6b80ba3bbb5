"""Host: the inputs of test_window_paths_gpu.py reach the routes they are named for.  window_paths.route restates which kernel
and which counting route of kernels/bam_window.hip takes each pass of 64 records; here every case must place the stated
passes on its route -- a condition on the inputs, not a measurement: a case that does not reach its route is the defect these
files close -- and route() itself is held to the oracle's window arithmetic.  Nothing here runs on the device."""
import numpy as np
import pytest

import orc
import window_paths as WP
from bam_synth import make_soa

CASES = WP.cases()
ENTRIES = ("host", "dev")


def _routes(name, entry, base_align=0):
    """[(label, [Pass ...])] for every batch of a case"""
    case = CASES[name]
    return [(label, WP.routes(soa, case.W, entry, base_align, cuts)) for label, soa, cuts in WP.batches(case)]


def _kinds(passes):
    return [p.route for p in passes]


# ---- the finding -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cigar", ["150M", "151M", "36M", "75M", "250M", "300M", "16M", "1M", "31M", "33M"])
@pytest.mark.parametrize("sort", [True, False])
def test_reads_of_one_length_never_reached_the_fast_kernel(cigar, sort):
    """test_bam_gpu.test_window_reads_of_one_length: 20,011 records over 2.7 Mb at W = 1000 put ~8 windows under a pass."""
    soa = make_soa(20_011, [("chrA", 2_000_000), ("chrB", 700_000)], 17, sort=sort, cigars=[cigar])
    t = WP.tally(WP.route(soa, 1000, WP.lim_of(soa, "host")))
    assert t == {"rest": 313}


def test_what_the_older_window_tests_reach():
    """test_window_every_nibble_code_and_window_seams reaches the fast kernel at ("150M", 20000) only, and never a span of more
    than one record; test_window_every_tail_of_a_span at five of its eleven sizes, with tails of 1, 4, 36 and 63 records."""
    for cigar, W in [("150M", 20000), ("151M", 1000), ("36M", 50), ("250M", 7)]:
        soa = make_soa(30_011, [("chrA", 1_500_000), ("chrB", 400_000)], 23, sort=True, cigars=[cigar])
        passes = WP.route(soa, W, WP.lim_of(soa, "host"))
        t = WP.tally(passes)
        assert (t == {"one": 376, "seam": 92, "rest": 1}) if W == 20000 else (t == {"rest": 469}), (cigar, W, t)
    tails = set()
    for n in [1, 63, 64, 65, 70, 109, 110, 128, 1024 + 68, 5 * 1024 + 100, 7 * 1024 + 1023]:
        soa = make_soa(n, [("chrA", 900_000)], 41 + n, sort=True, cigars=["150M"])
        fast = set()
        for W in (20000, 1000):
            passes = WP.route(soa, W, WP.lim_of(soa, "host"))
            fast |= {p.route for p in passes if p.route in WP.FAST}
            assert all(p.nvalid == 1 for p in passes if p.route == "span"), n
            if passes[-1].route in WP.FAST and passes[-1].nvalid < WP.WAVE:
                tails.add(passes[-1].nvalid)
        assert bool(fast) == (n in (1, 65, 1092, 5220, 8191)), (n, fast)
    assert tails == {1, 4, 36, 63}


# ---- a: every length ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["every_length", "every_length_lead5", "every_length_lead11"])
def test_every_length_has_three_fast_passes(name, entry):
    """192 records per length: three whole passes, spans for the even lengths from 32 on (256 bases only with head == 0)"""
    (_, passes), = _routes(name, entry)
    assert len(passes) == 3 * WP.MAX_LQ
    if entry == "dev":                                       # the batch's last pass under the exact end: 128 whole bytes per record
        assert passes[-1].route == "one"
        passes = passes[:-1]
    for i, p in enumerate(passes):
        lq = i // 3 + 1
        span = lq % 2 == 0 and lq >= 32 and (lq < 256 or p.head == 0)
        assert (p.route, p.lq, p.nvalid, p.steps) == ("span" if span else "one", lq, WP.WAVE, WP.steps_of(lq)), (i, p)
    if name == "every_length" and entry == "host":
        assert WP.tally(passes) == {"one": 429, "span": 339}
    # (64 records of 32 bases are one step of 1024 bytes only without a head)
    assert {p.steps for p in passes} == {1, 2, 4, 6, 7, 8} and {p.span_steps for p in passes if p.route == "span"} >= set(range(2, 9))
    assert {p.head for p in passes} == {CASES[name].soa.seq_off[0]}           # (192 records of any length are whole 16-byte pieces)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_length_off_the_lattice(entry):
    """200 records per length: mixed-length passes (rest) beside at least two fast ones for every length.  200 records are a
    whole number of 8-byte halves (heads 0 and 8 at most); 193 .. 205 put a head of every value in front of spans and of pieces."""
    for name, heads in (("every_length_200", None), ("every_length_ragged", set(range(16)))):
        (_, passes), = _routes(name, entry)
        t = WP.tally(passes)
        assert t["rest"] >= 200 and t["one"] >= 200 and t["span"] >= 200, t
        for lq in range(1, WP.MAX_LQ + 1):
            assert sum(p.route in WP.FAST and p.lq == lq for p in passes) >= 2, lq
        for kind in ("span", "one"):
            seen = {p.head for p in passes if p.route == kind}
            assert seen == heads if heads else seen <= {0, 8}, (name, kind, seen)


# ---- b: every tail -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lq", WP.TAIL_LENGTHS)
def test_every_tail_is_a_fast_pass_of_the_host_entry_and_straddles_the_dev_entrys_end(lq):
    """hpn_window_add has 16 bytes of slack behind the batch: every pass is fast.  hpn_window_add_dev's end is exact: a pass goes
    to k_window_rest when the 16-byte pieces of its last record reach beyond the batch's last byte (always the last pass, unless
    a record is a whole number of pieces; more passes when records are shorter than a piece), and is never a span."""
    nb = (lq + 1) // 2
    pieces = 16 * ((nb + 15) // 16)
    fast = "span" if lq % 2 == 0 and lq >= 32 else "one"
    seen = {b: set() for b in WP.TAIL_BASES}
    for (label, host), (_, dev) in zip(_routes("every_tail_%d" % lq, "host"), _routes("every_tail_%d" % lq, "dev")):
        n = int(label[2:])
        base = max(b for b in WP.TAIL_BASES if b < n)
        assert _kinds(host) == [fast] * len(host) and len(host) == base // WP.WAVE + 1, label
        ends = [(min(n, WP.WAVE * (i + 1)) - 1) * nb + pieces for i in range(len(dev))]     # where each pass's last piece ends
        assert _kinds(dev) == ["rest" if e > n * nb else fast if i + 1 < len(dev) else "one" for i, e in enumerate(ends)], label
        assert dev[-1].route == ("one" if nb % 16 == 0 else "rest")
        assert (host[-1].lq, host[-1].steps, host[-1].nvalid) == (lq, WP.steps_of(lq), n - base)
        seen[base].add(host[-1].nvalid)
    assert all(seen[b] == set(range(1, WP.WAVE + 1)) for b in WP.TAIL_BASES), seen


# ---- c: span alignment -------------------------------------------------------------------------------------------------

def test_spans_of_every_head_record_count_and_step_count():
    steps, heads_dev, aligns = set(), {lq: set() for lq in WP.SPAN_LENGTHS}, set()
    for lq in WP.SPAN_LENGTHS:
        for lead in range(16):
            name = "span_%d_lead%d" % (lq, lead)
            nvalids = []
            for label, passes in _routes(name, "host"):
                first, last = passes
                want = ["span" if lead + p.nvalid * (lq // 2) <= WP.SPAN_BYTES else "one" for p in passes]   # 8192 bytes and a head: nine steps
                assert (first.route, first.head, last.route, last.head, last.lq) == (want[0], lead, want[1], lead, lq), (name, label)
                assert want[0] == "span" or (lq == 256 and lead)
                steps |= {p.span_steps for p in passes if p.route == "span"}
                nvalids.append(last.nvalid)
            assert nvalids == WP.SPAN_NVALID
            for ba in CASES[name].base_aligns:
                aligns.add(ba)
                for label, passes in _routes(name, "dev", ba):
                    head = (lead + ba) & 15
                    assert (passes[0].route, passes[0].head) == ("one" if lq == 256 and head else "span", head), (name, ba, label)
                    assert passes[1].route != "span"             # the exact end: no 16 bytes behind the span
                    heads_dev[lq].add(head)
    assert steps == set(range(1, 9)) and aligns == set(range(16))
    assert all(h == set(range(16)) for h in heads_dev.values())


# ---- d: bytes that are not bases ---------------------------------------------------------------------------------------

def test_poison_lies_around_every_sequence():
    for name in CASES:
        if not name.startswith("gap"):
            continue
        soa = CASES[name].soa
        nb = (soa.l_qseq.astype(np.int64) + 1) // 2
        so = soa.seq_off.astype(np.int64)
        inside = np.zeros(len(soa.seq4), bool)
        for a, k in zip(so[:-1], nb):
            inside[a:a + k] = True
        assert (soa.seq4[~inside] == WP.POISON).all() and len(soa.seq4) == so[-1] + WP.TAIL
        assert (so[1:-1] - so[:-2] - nb[:-1] > 0).all() and so[-1] == so[-2] + nb[-1]
        assert len(np.unique(soa.seq4[inside])) == 256
        for entry in ENTRIES:
            (_, passes), = _routes(name, entry, 5 if entry == "dev" else 0)
            t = WP.tally(passes[:-1])
            assert set(t) == {"one"} and t["one"] == len(passes) - 1, (name, entry, t)     # apart: no span
    soa = CASES["every_length_lead5"].soa
    assert (soa.seq4[:5] == WP.POISON).all() and (soa.seq4[-WP.TAIL:] == WP.POISON).all()


# ---- e: skipped records ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("lq", WP.SKIP_LENGTHS)
def test_skipped_records_inside_dense_passes(lq, entry):
    (_, passes), = _routes("skipped_%d" % lq, entry)
    assert _kinds(passes) == WP.skipped_routes(lq, entry)
    assert [p.nok for p in passes] == [64, 63, 63, 63, 1, 0, 64, 63, 63, 63, 63, 64]
    assert lq != 36 or _kinds(passes)[7] == "one" != _kinds(passes)[0]      # the one skipped record keeps the pass off the span


# ---- f: seams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lq", WP.SEAM_LENGTHS)
def test_a_seam_behind_every_record(lq):
    for entry in ENTRIES:
        (_, passes), = _routes("seams_%d" % lq, entry)
        if entry == "dev":
            passes = passes[:-1]
        assert all((p.route, p.first, p.lq) == ("seam", k + 1, lq) for k, p in enumerate(passes))
    assert len(passes) == 62


def test_seam_cases_take_their_routes():
    host = {name: _routes(name, "host")[0][1] for name in CASES}
    assert _kinds(host["two_seams"]) == ["span", "rest", "span"]
    assert _kinds(host["width_one"]) == ["span", "span", "seam", "span"] * 2 + ["one", "one", "seam", "one"]
    assert all(p.route in WP.FAST for p in host["cached_window"]) and len(host["cached_window"]) == 11
    assert _kinds(host["short_wrap"]) == ["span", "span", "span", "seam", "one", "seam", "span"]
    assert _kinds(host["seam_out_of_target"]) == ["span", "rest"]
    assert _kinds(host["tid_out_of_range"]) == ["span", "rest", "span"]
    assert _kinds(host["negative_pos"]) == ["rest", "rest", "one"]
    for name in ("seam_out_of_target", "tid_out_of_range"):
        assert CASES[name].domain and orc.window_counts(CASES[name].soa, CASES[name].W)[0] != 0
    soa = CASES["short_wrap"].soa
    rc, off, bins, *_ = orc.window_counts(soa, 16)
    assert rc == 0 and int(off[-1]) > 65_541 and bins[65_536:].sum() == 0
    assert (bins[5], bins[0], bins[65_535]) == (3 * 64, 2 * 64 + 2 * 34, 2 * 30)
    soa = CASES["negative_pos"].soa
    rc, off, bins, *_ = orc.window_counts(soa, WP.W_DENSE)
    assert rc == 0 and bins[0] == 128 and (soa.pos < 0).sum() == 3


# ---- g, h --------------------------------------------------------------------------------------------------------------

def test_many_waves_on_one_window():
    (_, passes), = _routes("one_window_many_waves", "host")
    assert len(passes) == 1094 and _kinds(passes) == ["span"] * 1094 and passes[-1].nvalid == 70_000 % 64
    assert len(passes) > 4 * WP.SPAN_RECORDS // WP.WAVE * 16      # more spans of 1,024 records than a workgroup has waves


def test_later_calls_start_their_passes_elsewhere():
    case = CASES["several_calls"]
    assert all(c % WP.WAVE for c in case.cuts)
    for entry in ENTRIES:
        (_, passes), = _routes("several_calls", entry)
        t = WP.tally(passes)
        assert t["rest"] >= 250 and t["one"] >= 250 and t["span"] >= 200, t
        assert {p.nvalid for p in passes if p.route in WP.FAST} >= {1, 62, 2} or entry == "dev"


# ---- i: the raw route --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["samtools", "htsjdk97"])
def test_the_raw_route_reaches_the_fast_kernel_at_every_alignment(layout):
    raw = WP.raw_cases()
    heads = set()
    for half in (0, 1):
        case = raw["raw_every_length_%d" % half]
        passes = WP.route(WP.raw_view(case.soa, WP.RAW_SEED, layout), case.W, None)
        assert _kinds(passes) == ["one"] * len(passes) and len(passes) == 3 * 128   # (sequences lie apart in a record stream: no span)
        assert [p.lq for p in passes[::3]] == list(range(128 * half + 1, 128 * half + 129))
        heads |= {p.head for p in passes}
    assert heads == set(range(16))
    for lq in WP.SEAM_LENGTHS:
        case = raw["raw_seams_%d" % lq]
        passes = WP.route(WP.raw_view(case.soa, WP.RAW_SEED, layout), case.W, None)
        assert [(p.route, p.first) for p in passes] == [("seam", k) for k in range(1, 64)]
    for lq in WP.RAW_TAIL_LENGTHS:
        case = raw["raw_tails_%d" % lq]
        for label, soa, _ in WP.batches(case):
            passes = WP.route(WP.raw_view(soa, WP.RAW_SEED, layout), case.W, None)
            last = "span" if len(soa.tid) % 64 == 1 and lq % 2 == 0 and lq >= 32 else "one"      # (one record is a span of its own)
            assert _kinds(passes) == ["one"] * (len(passes) - 1) + [last] and passes[-1].nvalid == (len(soa.tid) - 1) % 64 + 1, label


# ---- route() against the oracle ----------------------------------------------------------------------------------------

def _random_inputs():
    refs = [("chrA", 300_000), ("chrB", 90_000), ("tiny", 300)]
    for seed, W, sort, cigars in [(1, 20000, True, ["150M"]), (2, 5000, True, ["36M"]), (3, 700, True, ["151M"]), (4, 64, True, ["250M"]),
                                  (5, 20000, False, ["150M"]), (6, 20000, True, None), (7, 3000, True, ["150M", "151M"])]:
        yield "s%d" % seed, make_soa(6_000, refs, seed, sort=sort, cigars=cigars), W
    soa = make_soa(6_000, [("long", 16 * 70_000)], 8, cigars=["150M"])
    soa.pos[:] = 16 * 65_530 + np.sort(soa.pos % (16 * 15))    # windows 65,530 .. 65,544: slots 65,530 .. 65,535, 0 .. 8
    yield "wrap", soa, 16
    soa = make_soa(6_000, [("c", 100_000)], 9, cigars=["100M"])
    soa.pos[::501] = 150_000                              # beyond the contig at W = 1000: the reference would write out of bounds
    yield "beyond", soa, 1000
    soa = make_soa(6_000, [("c", 100_000)], 10, cigars=["100M"])
    soa.tid[::389] = 1
    soa.pos[1::64] = -1
    yield "tid", soa, 1000
    for name in ("cached_window", "short_wrap", "seam_out_of_target", "width_one", "two_seams", "skipped_150"):
        yield name, CASES[name].soa, CASES[name].W


@pytest.mark.parametrize("name,soa,W", list(_random_inputs()), ids=lambda v: v if isinstance(v, str) else "")
def test_route_agrees_with_the_oracles_window_arithmetic(name, soa, W):
    """The oracle ((uint16)(pos / W), bam_sliding_count.c:117) on each pass alone: a fast pass counts in one slot (two for a
    seam: nfirst records in the first window's, the others in the next one's), an empty pass in none, and a pass the oracle
    refuses is never fast."""
    passes = WP.route(soa, W, WP.lim_of(soa, "host"))
    seen = set()
    for i, p in enumerate(passes):
        part = WP.cut(soa, WP.WAVE * i, min(len(soa.tid), WP.WAVE * (i + 1)))
        rc, off, bins, gc, ln, touched, nc = orc.window_counts(part, W)
        seen.add(p.route)
        if rc != 0:
            assert p.route == "rest", (i, p)
            continue
        slots = np.nonzero(bins)[0]
        assert nc == p.nok == bins.sum()
        if p.route == "empty":
            assert len(slots) == 0
        elif p.route in ("one", "span"):
            assert len(slots) == 1 and ln[slots[0]] == p.nok * p.lq and touched.sum() == 1, (i, p)
        elif p.route == "seam":
            ok = (part.tid >= 0) & ((part.flag & 4) == 0)
            t0, w0 = int(part.tid[ok][0]), int(part.pos[ok][0]) // W
            a, b = int(off[t0]) + (w0 & 0xffff), int(off[t0]) + ((w0 + 1) & 0xffff)
            assert sorted(slots) == sorted((a, b)) and (bins[a], bins[b]) == (p.first, p.nok - p.first), (i, p)
        else:
            lq = set(part.l_qseq.tolist())
            assert len(slots) > 1 or touched.sum() > 1 or len(lq) > 1 or max(lq) > WP.MAX_LQ or (part.pos < 0).any() or \
                part.seq_off[0] > part.seq_off[:-1].min(), (i, p)
    if name.startswith("s") and name[1:].isdigit():
        assert "rest" in seen
    if name in ("s1", "s2", "wrap"):
        assert seen >= {"one", "seam"}, seen


def test_route_on_hand_made_passes():
    """The rules on passes small enough to check by eye."""
    soa = WP.dense([(64, 150, 3), (10, 150, 3)], 1000)
    a, b = WP.route(soa, 1000, WP.lim_of(soa, "host"))
    assert a == WP.Pass("span", 150, 64, 6, 0, 5, 0, 64) and b == WP.Pass("span", 150, 10, 6, 0, 1, 0, 10)
    a, b = WP.route(soa, 1000, WP.lim_of(soa, "dev"), base_align=3)
    assert (a.route, a.head, b.route) == ("span", 3, "rest")             # 75 bytes: the last piece straddles the exact end
    a, b = WP.route(soa, 1000, None, base_align=3)
    assert (b.route, b.head, b.span_steps) == ("span", 3 + 64 * 75 & 15, 1)
    assert [p.route for p in WP.route(soa, 100, None)] == ["rest", "rest"]       # positions 3000 .. 3999 in both: ten windows
    assert [(p.route, p.first) for p in WP.route(soa, 500, None)] == [("seam", 32), ("seam", 5)]
    soa.l_qseq[5] = 149
    assert [p.route for p in WP.route(soa, 1000, None)] == ["rest", "span"]
    soa = WP.dense([(64, 151, 0)], 1000, lead=7, gap=2)
    (p,) = WP.route(soa, 1000, WP.lim_of(soa, "host"))
    assert p == WP.Pass("one", 151, 64, 6, 7, 0, 0, 64)
    soa = WP.dense([(64, 257, 0)], 1000)
    assert [p.route for p in WP.route(soa, 1000, None)] == ["rest"]
    assert [WP.steps_of(lq) for lq in (1, 32, 33, 64, 65, 96, 97, 128, 129, 150, 192, 193, 224, 225, 256)] == \
        [1, 1, 2, 2, 4, 4, 4, 4, 6, 6, 7, 8, 8, 8, 8]
