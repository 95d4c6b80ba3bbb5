"""K2 (`k_trim_scan`, `k_trim_copy`) and `k_qtrim_points` of kernels/fastq_trim.hip on every kept length, path, seam and trim
point, against the plain reference trim_ref.py (held against the C oracle in test_trim_ref_host.py, which also checks that the
inputs of trim_inputs.py hit the paths named here).  Bytes and integers: every comparison is exact.

  A  every kept count 16..1024 on the wave-uniform fast path of the copy (and the counts on both sides of it), at two source
     alignments; the thresholds 15/16 and 1024/1025 and every P = ceil(c0 / 16) class edge at five begins
  B  the same lengths on the mixed path; its 256-byte trips and the switch to byte copies below 16
  C  the fast path under per-record points (equal counts, irregular sources and destinations); the point edges
  D  scan tile seams (4096 records) with and without a window, and a batch larger than one grid sweep
  E  the device entry points writing into guarded allocations: not a byte outside [0, total) of an output changes
  F  k_qtrim_points with hits placed on the 64-byte chunk seams, thresholds 0, 256 and 2^32 - 1, quality bytes >= 128
"""
import numpy as np
import pytest

import trim_inputs as ti
import trim_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def _same(got, want, what, woff=None):
    """Exact equality of two flat arrays; woff (the reference's out_off) names the record a differing byte belongs to."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} elements, want {want.shape[0]}"
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    first = int(bad[0])
    where = ""
    if woff is not None:
        rec = int(np.searchsorted(woff, first, side="right")) - 1
        recs = np.unique(np.searchsorted(woff, bad, side="right") - 1)
        where = (f" = record {rec} (kept {int(woff[rec + 1] - woff[rec])} bytes) position {first - int(woff[rec])}; "
                 f"{len(recs)} records differ, first {recs[:6].tolist()}")
    raise AssertionError(f"{what}: {len(bad)} of {len(want)} differ, first at {first}{where}: got {got[first]}, want {want[first]}; "
                         f"last at {int(bad[-1])}")


def _same_cut(got, want, what):
    gseq, gqual, goff = got
    wseq, wqual, woff = want
    _same(goff, woff, what + " out_off")
    _same(gseq, wseq, what + " out_seq", woff)
    _same(gqual, wqual, what + " out_qual", woff)


def _check(ctx, b, S, E, what):
    want = trim_ref.cut(b.seq, b.qual, b.off, S, E)
    _same_cut(ctx.fastq_trim(b.seq, b.qual, b.off, S, E), want, f"{what} S={S} E={E}")
    return want


def _check_points(ctx, b, beg, end, what):
    want = trim_ref.cut_points(b.seq, b.qual, b.off, beg, end)
    _same_cut(ctx.fastq_trim_points(b.seq, b.qual, b.off, beg, end), want, what)
    return want


# ---- A. every kept length on uniform waves --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,E", ti.A_CUTS)
def test_every_kept_length_uniform(ctx, S, E):
    """Aligned groups of 64 equal reads, one group per length 0..1040 and 1279, 1280, 1281, 2053, 4100: every c0 of the fast path
    (P = 1..64 lanes per record, every overlap of the last piece), and uniform waves below 16 and above 1024 that must not take
    it.  S = 3 moves every source off the destinations' 16-byte phase."""
    _check(ctx, ti.case_a(), S, E, "A")


@pytest.mark.parametrize("kept", ti.A2_KEPT)
def test_fast_path_thresholds_and_begins(ctx, kept):
    """129 reads of 1100 bytes cut to `kept`: two uniform waves and a one-record wave on the mixed path."""
    for S in ti.A2_S:
        _, _, woff = _check(ctx, ti.case_a2(), S, S + kept, f"A2 kept={kept}")
        assert int(woff[-1]) == ti.A2_N * kept


# ---- B. the same lengths on the mixed path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ti.B_PREFIX)
def test_every_kept_length_mixed(ctx, prefix):
    """Case A behind 1, 17 or 63 records of 5 bytes: every wave straddles two lengths."""
    _check(ctx, ti.case_a(prefix), 0, ti.E_ALL, f"B prefix={prefix}")


def test_mixed_path_trips_and_byte_copies(ctx):
    """Groups of 63 and 65 equal records at 15/16/17 (byte copies below 16), 255..257, 271..273, 511..513 (one, two and three trips
    of the 256-byte loop and its overlapping last piece) and 1024/1025."""
    _check(ctx, ti.case_b_groups(), 0, ti.E_ALL, "B groups")


# ---- C. uniform waves under per-record points -----------------------------------------------------------------------------------
def test_uniform_waves_with_points(ctx):
    b = ti.case_c()
    _check_points(ctx, b, b.beg, b.end, "C")


def test_point_edges(ctx):
    """beg > len, end > len, end < beg, beg == end, 0xffffffff in either place, zero-length reads among them."""
    b = ti.case_c_edges()
    _, _, woff = _check_points(ctx, b, b.beg, b.end, "C edges")
    kept = np.diff(woff.astype(np.int64))
    for i, what in enumerate(b.hits["edges"]):
        if what != "end > len" and what != "beg = 0, end = 0xffffffff":
            assert kept[i] == 0, (i, what)


# ---- D. scan seams and the grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ti.D_SEAMS)
def test_scan_tile_seams(ctx, n):
    """Reads of 0..3 bytes cut to [1, 3): tiles whose aggregate is 0 among them; out_off[n] from the tile that holds record n - 1.
    Once as a batch of its own, once as the window off[5:] of a longer one."""
    b = ti.case_d_seam(n)
    alone = _check(ctx, ti.own(b, ti.D_LEAD), *ti.D_SEAM_CUT, f"D n={n} own")
    window = _check(ctx, ti.Batch(b.seq, b.qual, b.off[ti.D_LEAD:], b.hits), *ti.D_SEAM_CUT, f"D n={n} window")
    assert len(alone[2]) == n + 1 and np.array_equal(alone[2], window[2])


def test_more_than_one_grid_sweep(ctx):
    """n_cu * 8 * 256 + 4096 + 77 records of 0..40 bytes: the waves of the copy and of k_qtrim_points take a second turn."""
    import torch
    b = ti.case_d_grid(torch.cuda.get_device_properties(0).multi_processor_count)
    _check(ctx, b, *ti.D_GRID_CUT, "D grid")
    wb, we = trim_ref.qtrim_points_flat(b.qual, b.off, ti.D_GRID_T)
    gb, ge = ctx.fastq_qtrim_points(b.qual, b.off, ti.D_GRID_T)
    _same(gb, wb, "D grid qtrim beg")
    _same(ge, we, "D grid qtrim end")


# ---- E. the device entry points, with guards ------------------------------------------------------------------------------------
GUARD, FILL = 256, 0xA5
OUT_AT, IN_AT = (0, 1, 3, 8, 15), (0, 1, 7)


class _Guarded:
    """`nbytes` of payload at byte GUARD + at of a device allocation filled with 0xA5, GUARD more bytes behind it.  Everything the
    kernels are given lies inside the allocation, the guards included."""

    def __init__(self, nbytes, at, data=None):
        import torch
        self.lo, self.n = GUARD + at, nbytes
        self.t = torch.full((GUARD + at + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if data is not None and nbytes:
            self.t[self.lo:self.lo + nbytes] = torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()).cuda()
        self.ptr = self.t.data_ptr() + self.lo

    def check(self, want, what):
        """The payload starts with `want`; every other byte of the allocation is still 0xA5."""
        got = self.t.cpu().numpy()
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        front, body, rest = got[:self.lo], got[self.lo:self.lo + len(want)], got[self.lo + len(want):]
        assert (front == FILL).all(), f"{what}: {int((front != FILL).sum())} guard bytes in front changed, nearest {self.lo - int(np.flatnonzero(front != FILL)[-1])} before the output"
        assert (rest == FILL).all(), f"{what}: {int((rest != FILL).sum())} bytes behind the output's end changed, first {int(np.flatnonzero(rest != FILL)[0])} past it"
        return body


def _dev_cut(ctx, b, S, E, what):
    """The cut through hpn_fastq_trim_dev (fixed cycles) or hpn_fastq_trim_points_dev (b.beg / b.end), outputs at every offset of
    OUT_AT and inputs at every offset of IN_AT of their allocations.  The offsets, the points and out_off are 8- and 4-byte words
    and stay aligned (the ABI takes them as uint64_t * / uint32_t *); they get guard words all the same."""
    import torch
    assert int(b.off[0]) == 0
    n, nbytes = len(b.off) - 1, int(b.off[-1])
    points = b.beg is not None
    want = trim_ref.cut_points(b.seq, b.qual, b.off, b.beg, b.end) if points else trim_ref.cut(b.seq, b.qual, b.off, S, E)
    wseq, wqual, woff = want
    total = int(woff[-1])
    for ia in IN_AT:
        d_seq, d_qual = _Guarded(nbytes, ia, b.seq), _Guarded(nbytes, IN_AT[-1] - ia, b.qual)
        d_off = _Guarded(8 * (n + 1), 0, b.off)
        d_beg = _Guarded(4 * n, 0, b.beg) if points else None
        d_end = _Guarded(4 * n, 0, b.end) if points else None
        for oa in OUT_AT:
            w = f"{what} inputs at +{ia}, outputs at +{oa}"
            o_seq, o_qual, o_off = _Guarded(nbytes, oa), _Guarded(nbytes, OUT_AT[-1] - oa), _Guarded(8 * (n + 1), 0)
            torch.cuda.synchronize()
            if points:
                ctx.fastq_trim_points_dev(d_seq.ptr, d_qual.ptr, d_off.ptr, n, d_beg.ptr, d_end.ptr, o_seq.ptr, o_qual.ptr, o_off.ptr)
            else:
                ctx.fastq_trim_dev(d_seq.ptr, d_qual.ptr, d_off.ptr, n, S, E, o_seq.ptr, o_qual.ptr, o_off.ptr)
            ctx.sync()
            goff = o_off.check(woff, w + " out_off").view(np.uint64)
            _same(goff, woff, w + " out_off")
            assert int(goff[n]) == total
            _same(o_seq.check(wseq, w + " out_seq"), wseq, w + " out_seq", woff)
            _same(o_qual.check(wqual, w + " out_qual"), wqual, w + " out_qual", woff)
        for g, src, name in ((d_seq, b.seq, "seq"), (d_qual, b.qual, "qual"), (d_off, b.off, "off")):
            _same(g.check(src, f"{what} input {name}"), np.ascontiguousarray(src).view(np.uint8).reshape(-1), f"{what} input {name} unchanged")


@pytest.mark.parametrize("name", list(ti.DEV_FIXED))
def test_trim_dev_writes_only_its_output(ctx, name):
    """(a) 150-byte reads cut to [5, 140), (b) kept 16, (c) kept 1024, (d) kept 1025, (e) lengths 0..300: 193 records each."""
    _, _, S, E = ti.DEV_FIXED[name]
    _dev_cut(ctx, ti.case_dev(name), S, E, f"E {name}")


def test_trim_points_dev_writes_only_its_output(ctx):
    """(f) the case-C batch: every fast-path lane count with irregular sources, through hpn_fastq_trim_points_dev."""
    _dev_cut(ctx, ti.case_c(), 0, 0, "E points")


@pytest.mark.parametrize("points", [False, True])
def test_trim_dev_empty_batch(ctx, points):
    """n = 0: the scan's one tile holds no record and still writes out_off[0] = 0, and nothing else is written.  (Through the host
    entry points out_off[0] comes back from scratch whose first word every earlier call left at 0.)"""
    import torch
    d_seq, d_qual, d_off, d_pts = _Guarded(0, 1), _Guarded(0, 7), _Guarded(8, 0, np.array([9], np.uint64)), _Guarded(0, 0)
    o_seq, o_qual, o_off = _Guarded(0, 3), _Guarded(0, 15), _Guarded(8, 0)
    torch.cuda.synchronize()
    if points:
        ctx.fastq_trim_points_dev(d_seq.ptr, d_qual.ptr, d_off.ptr, 0, d_pts.ptr, d_pts.ptr, o_seq.ptr, o_qual.ptr, o_off.ptr)
    else:
        ctx.fastq_trim_dev(d_seq.ptr, d_qual.ptr, d_off.ptr, 0, 2, 30, o_seq.ptr, o_qual.ptr, o_off.ptr)
    ctx.sync()
    zero = np.zeros(1, np.uint64)
    _same(o_off.check(zero, "n = 0 out_off").view(np.uint64), zero, "n = 0 out_off")
    for g, name in ((o_seq, "out_seq"), (o_qual, "out_qual"), (d_seq, "seq"), (d_qual, "qual"), (d_pts, "points")):
        g.check(np.zeros(0, np.uint8), f"n = 0 {name}")
    assert d_off.check(np.array([9], np.uint64), "n = 0 off").view(np.uint64).tolist() == [9]


@pytest.mark.parametrize("which", ["F directed T=53", "E mixed T=53", "E mixed T=256"])
def test_qtrim_points_dev_writes_only_its_output(ctx, which):
    import torch
    b, T = (ti.case_f_directed(53), 53) if which.startswith("F") else (ti.case_dev("e_mixed_0_300"), int(which.split("=")[1]))
    n, nbytes = len(b.off) - 1, int(b.off[-1])
    wb, we = trim_ref.qtrim_points(b.qual, b.off, T)
    d_off = _Guarded(8 * (n + 1), 0, b.off)
    for ia in IN_AT:
        d_qual = _Guarded(nbytes, ia, b.qual)
        o_beg, o_end = _Guarded(4 * n, 0), _Guarded(4 * n, 0)
        torch.cuda.synchronize()
        ctx.fastq_qtrim_points_dev(d_qual.ptr, d_off.ptr, n, T, o_beg.ptr, o_end.ptr)
        ctx.sync()
        _same(o_beg.check(wb, f"{which} beg").view(np.uint32), wb, f"{which} qual at +{ia} beg")
        _same(o_end.check(we, f"{which} end").view(np.uint32), we, f"{which} qual at +{ia} end")
        d_qual.check(b.qual, f"{which} input qual")


# ---- F. k_qtrim_points, directed ------------------------------------------------------------------------------------------------
def _check_qtrim(ctx, b, T, what):
    wb, we = trim_ref.qtrim_points(b.qual, b.off, T)
    gb, ge = ctx.fastq_qtrim_points(b.qual, b.off, T)
    _same(gb, wb, f"{what} T={T} beg")
    _same(ge, we, f"{what} T={T} end")
    _check_points(ctx, b, gb, ge, f"{what} T={T} cut at the points")
    return wb, we


@pytest.mark.parametrize("T", ti.F_T)
def test_qtrim_points_directed(ctx, T):
    """Lengths on both sides of the 64-byte chunks; no hit, all hits, one hit and two hits at 0, 1, 62..65, 127, 128, len - 2,
    len - 1: the first hit kept across chunks, the last hit from the last chunk that has one.  Hits are T exactly, the rest T - 1
    (T = 128 and 255: quality bytes with the top bit set)."""
    _check_qtrim(ctx, ti.case_f_directed(T), T, "F directed")


@pytest.mark.parametrize("T", ti.F_RANDOM_T)
def test_qtrim_points_random_bytes(ctx, T):
    """Bytes over 0..255: T = 0 keeps every read whole, T = 256 and 2^32 - 1 keep nothing (the comparison is unsigned, 32 bits)."""
    b = ti.case_f_random()
    wb, we = _check_qtrim(ctx, b, T, "F random")
    if T > 255:
        assert not wb.any() and not we.any()
    if T == 0:
        assert np.array_equal(we, np.diff(b.off.astype(np.int64)).astype(np.uint32))
