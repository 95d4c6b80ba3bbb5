"""GPU parity of k_window_add's fast pass (kernels/bam_window.hip) at every read length, tail and seam: the cases of
tests/window_paths.py -- which test_window_paths_host.py holds to the routes they are named for -- through hpn_window_add AND
hpn_window_add_dev (and, where named, the raw route), bit-exact against the oracle on bins, gc, len, touched and n_count.
Integers only: there is no tolerance anywhere.

Around every sequence the _dev entry's tensor holds 0x24 (a C and a G): in front of seq_off[0], in every gap between sequences
and in 64 bytes behind seq_off[n].  None of them is a base."""
import ctypes as C

import numpy as np
import pytest

import orc
import window_paths as WP
from highperformancengs_amd import _lib
from highperformancengs_amd.api import _ptr

pytestmark = pytest.mark.gpu

CASES = WP.cases()
RAW = WP.raw_cases()
FRONT = 16                # bytes of POISON in front of the _dev entry's seq4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


class _Dev:
    """a batch on the device: tensors (or views of them) under hpn_bam_batch's names"""

    def __init__(self, soa, base_align):
        import torch
        for f in ("tid", "pos", "l_qseq"):
            setattr(self, f, torch.from_numpy(np.ascontiguousarray(getattr(soa, f))).cuda())
        self.flag = torch.from_numpy(np.ascontiguousarray(soa.flag).view(np.int32)).cuda()
        self.seq_off = torch.from_numpy(np.ascontiguousarray(soa.seq_off).view(np.int64)).cuda()
        self.buf = torch.full((FRONT + base_align + len(soa.seq4),), WP.POISON, dtype=torch.uint8, device="cuda")
        self.seq4 = self.buf[FRONT + base_align:]
        self.seq4.copy_(torch.from_numpy(soa.seq4))
        assert self.seq4.data_ptr() & 15 == base_align and int(soa.seq_off[-1]) + WP.TAIL == len(soa.seq4)
        torch.cuda.synchronize()

    def part(self, a, b):
        d = object.__new__(_Dev)
        for f in ("tid", "pos", "l_qseq", "flag"):
            setattr(d, f, getattr(self, f)[a:b])
        d.seq_off, d.seq4 = self.seq_off[a:b + 1], self.seq4
        return d


def _counts(ctx, off, W, parts, dev):
    """hpn_window_begin, one add per part, hpn_window_finish"""
    off = np.ascontiguousarray(off, np.uint64)
    nt, tot = len(off) - 1, int(off[-1])
    ctx._ck(ctx.L.hpn_window_begin(ctx.h, nt, _ptr(off), W), "hpn_window_begin")
    add = ctx.L.hpn_window_add_dev if dev else ctx.L.hpn_window_add
    for p in parts:
        keep = []
        ctx._ck(add(ctx.h, C.byref(ctx._batch(p, keep))), "hpn_window_add")
    bins, gc, ln = np.zeros(tot, np.uint32), np.zeros(tot, np.uint64), np.zeros(tot, np.uint32)
    touched, nc = np.zeros(nt, np.uint8), C.c_uint64(0)
    ctx._ck(ctx.L.hpn_window_finish(ctx.h, _ptr(bins), _ptr(gc), _ptr(ln), _ptr(touched), C.byref(nc)), "hpn_window_finish")
    return bins, gc, ln, touched, nc.value


def _same(got, want, what):
    bins, gc, ln, touched, nc = got
    _, _, wb, wg, wl, wt, wn = want
    for name, g, w in (("bins", bins, wb), ("gc", gc, wg), ("len", ln, wl), ("touched", touched, wt)):
        if not np.array_equal(g, w):
            at = np.nonzero(g != w)[0]
            raise AssertionError("%s: %s differs in %d slots, first %d: got %d, want %d" % (what, name, len(at), at[0], g[at[0]], w[at[0]]))
    assert nc == wn, (what, nc, wn)


def _edges(n, cuts):
    e = [0] + list(cuts or []) + [n]
    return list(zip(e[:-1], e[1:]))


def _run(ctx, case, name):
    """every batch of a case through both entries (the _dev entry at every base_align of the case)"""
    import highperformancengs_amd as hp
    want = {label: orc.window_counts(soa, case.W) for label, soa, _ in WP.batches(case)}
    assert all((w[0] != 0) == case.domain for w in want.values())
    if case.domain:
        (label, soa, _), = WP.batches(case)
        for dev, part in ((False, soa), (True, _Dev(soa, 0))):
            with pytest.raises(hp.HpnError) as e:
                _counts(ctx, orc.window_offsets(soa.refs, case.W), case.W, [part], dev)
            assert e.value.status == _lib.E_DOMAIN
        return
    for label, soa, cuts in WP.batches(case):
        parts = [WP.cut(soa, a, b) for a, b in _edges(len(soa.tid), cuts)]
        _same(_counts(ctx, want[label][1], case.W, parts, False), want[label], "%s %s hpn_window_add" % (name, label))
    for ba in case.base_aligns:
        whole = _Dev(case.soa, ba)
        for label, soa, cuts in WP.batches(case):
            parts = [whole.part(a, b) for a, b in _edges(len(soa.tid), cuts)]
            _same(_counts(ctx, want[label][1], case.W, parts, True), want[label], "%s %s hpn_window_add_dev, seq4 at +%d" % (name, label, ba))


# ---- a: every length ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in WP.EVERY_LENGTH])
def test_every_length_in_one_batch(ctx, name):
    """l_qseq 1 .. 256, one window per length, in one batch: a wave meets changing lengths and rebuilds its layout (masks, lane to
    piece map, step counts, the odd lengths' padding clip); a wrong length shows in its own window."""
    _run(ctx, CASES[name], name)


# ---- b: every tail -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lq", WP.TAIL_LENGTHS)
def test_every_tail_behind_a_pass_and_behind_a_span(ctx, lq):
    """the batch's last pass holds 1 .. 64 records, behind one whole pass and behind a whole span of 1,024; under the _dev
    entry's exact end the last pieces straddle it and the pass goes to k_window_rest"""
    _run(ctx, CASES["every_tail_%d" % lq], "every_tail_%d" % lq)


# ---- c: span alignment -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lq", WP.SPAN_LENGTHS)
def test_spans_at_every_alignment(ctx, lq):
    """back-to-back even lengths with 0 .. 15 bytes in front, 64 / 63 / 17 / 1 records in the span, the seq4 tensor itself at
    +0 .. +15: the span's first and last 16-byte piece are masked by where the pass's bytes begin and end"""
    for lead in range(16):
        name = "span_%d_lead%d" % (lq, lead)
        _run(ctx, CASES[name], name)


# ---- d: bytes that are not bases ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("gap")])
def test_bytes_between_sequences_are_not_counted(ctx, name):
    _run(ctx, CASES[name], name)


# ---- e: skipped records ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lq", WP.SKIP_LENGTHS)
def test_skipped_records_inside_dense_passes(ctx, lq):
    """flag 4 or tid -1 on lane 0, on lane 63, on all but one record, on every record, on one record of a span-eligible pass; a
    skipped record of another length, and one whose sequence lies in front of lane 0's (window_paths.SKIP_SCENES)"""
    _run(ctx, CASES["skipped_%d" % lq], "skipped_%d" % lq)


# ---- f: seams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lq", WP.SEAM_LENGTHS)
def test_a_seam_behind_every_record(ctx, lq):
    _run(ctx, CASES["seams_%d" % lq], "seams_%d" % lq)


@pytest.mark.parametrize("name", ["two_seams", "width_one", "cached_window", "short_wrap", "negative_pos"])
def test_windows_across_passes(ctx, name):
    """two boundaries under one pass; W = 1; the cached window (5, 5, 3, 5; target 0 then target 1 at the same positions); slots
    that wrap like unsigned short on the fast routes; pos -1"""
    _run(ctx, CASES[name], name)


@pytest.mark.parametrize("name", ["seam_out_of_target", "tid_out_of_range"])
def test_domain_errors_out_of_dense_passes(ctx, name):
    _run(ctx, CASES[name], name)


# ---- g, h --------------------------------------------------------------------------------------------------------------

def test_many_waves_flush_onto_one_window(ctx):
    _run(ctx, CASES["one_window_many_waves"], "one_window_many_waves")


def test_several_calls_between_begin_and_finish(ctx):
    """every length again, cut at records 1, 63, 65, 1000 and 1025: later calls start their passes at other alignments"""
    _run(ctx, CASES["several_calls"], "several_calls")


# ---- i: the raw route --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(RAW))
def test_raw_route(ctx, name):
    """the same records as BAM files (names of cycling lengths: sequences at every alignment) through hpn_window_add_raw_dev"""
    import test_bam_raw_layouts_gpu as RL
    case = RAW[name]
    for label, soa, _ in WP.batches(case):
        RL._raw_check(ctx, soa, WP.RAW_SEED, window=[case.W])
