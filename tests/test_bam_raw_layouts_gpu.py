"""GPU parity of the in-place record route (what bam2depth, bam2wig and bam_sliding_count run: BGZF blocks inflated on the device,
records indexed where they lie by kernels/bam_raw.hip, depth through RawRecs, windows through k_raw_fields) against the oracle's
dense model, on the record layouts of real BAM files (tests/bam_layouts.py): read names of 1 .. 254 characters, auxiliary fields
of every type, CIGARs of up to 65,535 operations, long reads, records > 64 KiB -- in samtools' block layout and htsjdk's.

* the adversarial battery of tests/test_bam_gpu.py and tests/test_depth_sweep_gpu.py (which runs through the SoA entry points
  only) replayed through the raw route;
* what only the raw route has: n_cigar read in place, CIGAR starts at every offset, far breakpoints found by walking each
  record's CIGAR, sequences read at stream offsets, guessed block starts refuted by the proof, records carried from call to call.
Every call's index must be exact (no flag, no tail, the record count) before any result is compared."""
import ctypes as C

import numpy as np
import pytest

import bam_layouts as BL
import orc
from bam_synth import make_soa
from highperformancengs_amd import _lib

pytestmark = pytest.mark.gpu

LAYOUTS = ("samtools", "htsjdk97")
FAR_CIGARS = ["150M", "50M2047N50M", "50M2048N50M", "30M1999D20M100N40M", "10M20000N10M30000N10M", "5M100000D5M",
              "1M16383N1M", "40M2I108M", "10S140M", "2049M", "17000M", "1N1M", "40000M"]
SWEEP_FAR = ["150M", "50M2047N50M", "50M2048N50M", "30M1999D20M100N40M", "10M20000N10M30000N10M", "5M100000D5M"]
SWEEP_NEAR = ["150M", "40M2I108M", "60M5D90M", "10S140M", "1M", "70M500D70M", "5=5X", "20M3000I20M", "600M"]
SWEEP_EDGE = ["150M", "40M2I108M", "50M1900N50M", "70M500D70M", "5=5X"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def _stream(soa, seed, aux="pool"):
    n = len(soa.tid)
    ax = BL.pick_aux(seed, n) if aux == "pool" else BL.embedded_chain_aux(seed, n) if aux == "chain" else None
    return BL.encode_stream(soa, BL.cycling_names(n), ax, qual_seed=seed)


def _pack(layout, data, bounds):
    if layout == "samtools":
        return BL.pack_samtools(data, bounds)
    return BL.bgzf_pack(data, int(layout[len("htsjdk"):]), level=1, eof=True)


def _in_domain(soa, window_Ws=()):
    """the inputs' own conditions: every M end below 2^28 (orc at rc 0) and every window's G/C sum below 2^24"""
    for W in window_Ws:
        rc, _, _, gc, *_ = orc.window_counts(soa, W)
        assert rc == 0 and int(gc.max(initial=0)) < 1 << 24, W


def _index(ctx, raw, n):
    d_raw, info, keep = BL.to_device(ctx, raw)
    assert info.flags & 3 == 0 and info.tail_bytes == 0 and info.n_records == n, (info.flags, info.tail_bytes, info.n_records, n)
    return d_raw, keep


def _raw_check(ctx, soa, seed, depth=(), window=(), layouts=LAYOUTS, aux="pool"):
    """soa as a BAM file of every layout through the raw route: depth for each (W, mask), windows for each W"""
    _in_domain(soa, window)
    want_d = {(W, mask, tid): orc.depth_target(soa, tid, W, mask) for W, mask in depth for tid in range(len(soa.refs))}
    want_w = {W: orc.window_counts(soa, W) for W in window}
    assert all(w[0] == 0 for w in want_d.values()) and all(w[0] == 0 for w in want_w.values())
    data, bounds = _stream(soa, seed, aux)
    for layout in layouts:
        d_raw, keep = _index(ctx, _pack(layout, data, bounds), len(soa.tid))
        for (W, mask, tid), (_, wruns, wbins) in want_d.items():
            runs, win = ctx.depth_target_raw(d_raw, tid, soa.refs[tid][1], W, mask)
            assert len(runs) == len(wruns) and np.array_equal(runs, wruns), (layout, tid, W, mask, len(runs), len(wruns))
            assert np.array_equal(win.astype(np.float64), wbins), (layout, tid, W, mask)
        for W, (_, off, wb, wg, wl, wt, wn) in want_w.items():
            bins, gc, ln, touched, nc = ctx.window_counts_raw(d_raw, off, W)
            assert np.array_equal(bins, wb) and np.array_equal(gc, wg) and np.array_equal(ln, wl), (layout, W)
            assert np.array_equal(touched, wt) and nc == wn, (layout, W)


# ---- the SoA battery of tests/test_bam_gpu.py, replayed --------------------------------------------------------------

@pytest.mark.parametrize("n,seed,sort", [(8_000, 31, True), (8_000, 32, False), (300, 33, True)])
def test_far_breakpoints(ctx, n, seed, sort):
    soa = make_soa(n, [("chrA", 1_500_000), ("chrB", 200_000)], seed, sort=sort, cigars=FAR_CIGARS, max_start_frac=0.9)
    _raw_check(ctx, soa, seed, depth=[(20000, 0x704), (20000, 0x4), (313, 0x4)], window=[20000])


def test_tile_edges(ctx):
    T, R = 16384, 2048
    starts = sorted({max(0, t * T + d) for t in range(0, 7) for d in (-R - 1, -R, -R + 1, -151, -150, -149, -1, 0, 1)} | {0, 1})
    recs = [(0, p, 0, cg, 0, None) for p in starts for cg in ("150M", "1M", "10M2037N1M", "10M2038N1M", "10M2039N1M", "100M100D100M")]
    _raw_check(ctx, BL.soa_from([("c", 120_000)], recs), 7, depth=[(1000, 0x704), (1000, 0x4)], window=[1000])


def test_dense_change_points(ctx):
    rng = np.random.default_rng(77)
    pos, cg = [], []
    for p in range(1000, 40_000):
        for _ in range(1 + p % 2):
            pos.append(p), cg.append("31M")
    for p in range(40_000, 90_000):
        pos.append(p), cg.append("%dM" % rng.integers(1, 40))
    pos.append(95_000), cg.append("60000M")
    for p in range(100_000, 131_072, 3):
        pos.append(p), cg.append("2M")
    for e in (16384, 65536, 131072, 196608):
        for dlt in (-2, -1, 0, 1):
            pos.append(e + dlt + 200_000 - e % 7), cg.append("1M")
        pos.append(e + 150_000 - 100), cg.append("100M")
        pos.append(e + 150_000), cg.append("100M")
    order = np.argsort(np.array(pos), kind="stable")
    recs = [(0, int(pos[i]), 0, cg[i], 0, None) for i in order]
    _raw_check(ctx, BL.soa_from([("d", 400_000)], recs), 8, depth=[(1, 0x704), (1000, 0x704)], window=[1, 1000])


@pytest.mark.parametrize("cigar", ["1M", "16M", "150M", "151M", "250M", "300M"])
@pytest.mark.parametrize("sort", [True, False])
def test_reads_of_one_length(ctx, cigar, sort):
    soa = make_soa(10_011, [("chrA", 2_000_000), ("chrB", 700_000)], 17, sort=sort, cigars=[cigar])
    _raw_check(ctx, soa, 17, depth=[(1000, 0x704)], window=[1000])


@pytest.mark.parametrize("cigar,W", [("150M", 20000), ("151M", 1000), ("36M", 50), ("250M", 7)])
def test_every_nibble_code_with_flag_and_unmapped_stretches(ctx, cigar, W):
    soa = make_soa(30_011, [("chrA", 1_500_000), ("chrB", 400_000)], 23, sort=True, cigars=[cigar])
    soa.seq4[:] = np.random.default_rng(5).integers(0, 256, soa.seq4.size, dtype=np.uint8)
    soa.flag[1000:1200] = 4
    soa.flag[5000:9000:7] |= 4
    soa.tid[20_000:20_100] = -1
    _raw_check(ctx, soa, 23, depth=[(W, 0x704), (W, 0x4)], window=[W])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70, 109, 110, 128, 1024 + 68, 5 * 1024 + 100, 7 * 1024 + 1023])
def test_every_tail_of_a_span(ctx, n):
    soa = make_soa(n, [("chrA", 900_000)], 41 + n, sort=True, cigars=["150M"])
    _raw_check(ctx, soa, n, window=[20000, 1000])


def test_window_index_wraps_like_unsigned_short(ctx):
    soa = make_soa(20_000, [("long", 10_000_000)], 9)
    _raw_check(ctx, soa, 9, depth=[(20000, 0x704)], window=[100])


def test_domain_errors_are_the_soa_routes(ctx):
    """Where tests/test_bam_gpu.py asserts HPN_E_DOMAIN for a SoA batch, the raw route gives the same status."""
    import highperformancengs_amd as hp
    soa = make_soa(10, [("big", 300_000_000)], 1, cigars=["100M"])
    soa.pos[:] = np.arange(10) * 1000 + 268_435_400       # ends beyond 2^28
    soa2 = make_soa(10, [("c", 1000)], 1)
    soa2.pos[3] = 5000                                      # beyond the contig: window 50 of 11
    assert orc.window_counts(soa2, 100)[0] != 0
    for layout in LAYOUTS:
        data, bounds = _stream(soa, 1)
        d_raw, keep = _index(ctx, _pack(layout, data, bounds), 10)
        with pytest.raises(hp.HpnError) as e:
            ctx.depth_target_raw(d_raw, 0, soa.refs[0][1], 20000)
        assert e.value.status == _lib.E_DOMAIN
        data, bounds = _stream(soa2, 2)
        d_raw, keep = _index(ctx, _pack(layout, data, bounds), 10)
        with pytest.raises(hp.HpnError) as e:
            ctx.window_counts_raw(d_raw, orc.window_offsets(soa2.refs, 100), 100)
        assert e.value.status == _lib.E_DOMAIN


# ---- several calls, the unfinished record carried (host/bam_gpu.hpp) --------------------------------------------------

def _calls(ctx, raw, data, bounds, cuts, each=None):
    """The file's record blocks in calls [cuts[k], cuts[k + 1]) (block numbers from the one the first record starts in); the
    bytes of the record a call ends in go in front of the next call's stream.  Every call's index is checked against the
    stream: the records whole in it, the bytes of the unfinished one.  each(d_raw) runs after every index."""
    import torch
    blks, start, first = _block_starts(raw, bounds)
    hl = int(bounds[0])
    d_comp = torch.from_numpy(np.frombuffer(raw + bytes(64), np.uint8).copy()).cuda()
    keep, front, done, begin = [], b"", 0, hl
    cuts = [first + c for c in cuts]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        table = np.zeros((hi - lo, 3), np.uint64)
        outo = len(front)
        for i, (a, n, isz) in enumerate(blks[lo:hi]):
            table[i] = (a, n | (isz << 32), outo)
            outo += isz
        d_blocks = torch.from_numpy(table.view(np.int64)).cuda()
        d_out = torch.zeros(outo + 64, dtype=torch.uint8, device="cuda")
        if front:
            d_out[:len(front)] = torch.from_numpy(np.frombuffer(front, np.uint8).copy()).cuda()
        d_status = torch.zeros(hi - lo, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.bgzf_inflate_dev(d_comp, d_blocks, hi - lo, d_out, d_status)
        info = ctx.bam_raw_index_dev(d_out, d_blocks, hi - lo, begin - start[lo] if lo == first else 0, d_status)
        end = start[hi - 1] + blks[hi - 1][2] if hi > lo else start[lo]
        whole = int(np.searchsorted(bounds, end, "right")) - 1          # records [done, whole) end at or before `end`
        tail = end - int(bounds[whole]) if whole < len(bounds) - 1 else 0
        assert info.flags & 3 == 0 and info.n_records == whole - done and info.tail_bytes == tail, \
            (lo, hi, info.flags, info.n_records, whole - done, info.tail_bytes, tail)
        if each is not None:
            each(d_out)
        stream = bytes(d_out[:outo].cpu().numpy())
        assert stream[:len(front)] == front and stream[len(front):] == data[start[lo]:end]
        front = stream[len(stream) - tail:] if tail else b""
        keep += [d_blocks, d_out, d_status]
        done = whole
    assert done == len(bounds) - 1 and not front
    return keep


def _block_starts(raw, bounds):
    """-> (blocks, stream offset of every block, the block the first record starts in -- as BL.to_device picks it)"""
    blks, start, acc = BL.blocks(raw), [], 0
    for _, _, isz in blks:
        start.append(acc)
        acc += isz
    first = 0
    while first < len(blks) - 1 and start[first] + blks[first][2] <= bounds[0]:
        first += 1
    return blks, start, first


def _record_blocks(raw, bounds):
    """number of blocks from the one the first record starts in"""
    blks, _, first = _block_starts(raw, bounds)
    return len(blks) - first


@pytest.mark.parametrize("cigars,n,seed", [(SWEEP_FAR, 30_000, 1), (SWEEP_EDGE, 30_000, 2), (SWEEP_NEAR, 30_000, 3)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sweep_across_raw_calls(ctx, cigars, n, seed, layout):
    """test_depth_sweep_gpu.py's record sets in 2 .. 5 hpn_depth_add_raw_dev calls between one hpn_depth_begin and
    hpn_depth_finish, cut at random blocks: the sweep's frontier moves across calls on the raw route too."""
    refs = [("chrA", 5_000_000), ("chrB", 3_000_000 + 12_345)]
    soa = make_soa(n, refs, seed, cigars=cigars)
    data, bounds = _stream(soa, seed)
    raw = _pack(layout, data, bounds)
    nb = _record_blocks(raw, bounds)
    rng = np.random.default_rng(seed)
    for pieces in (2, 3, 5):
        cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, nb), pieces - 1, replace=False)) + [nb]
        for tid, (name, tlen) in enumerate(refs):
            assert ctx.L.hpn_depth_begin_w(ctx.h, tid, tlen, 0x704, 20000) == 0
            keep = _calls(ctx, raw, data, bounds, cuts,
                          each=lambda d: ctx._ck(ctx.L.hpn_depth_add_raw_dev(ctx.h, ctx_ptr(d)), "hpn_depth_add_raw_dev"))
            v = C.c_uint64(0)
            assert ctx.L.hpn_depth_progress(ctx.h, C.byref(v)) == 0
            if cigars is not SWEEP_FAR:                     # (a reach walked record by record, <= 2048: the calls are swept)
                assert v.value > 0, (name, pieces)
            runs, win = ctx.depth_finish(tlen, 20000)
            rc, wruns, wbins = orc.depth_target(soa, tid, 20000, 0x704)
            assert rc == 0 and len(runs) == len(wruns) and np.array_equal(runs, wruns), (name, pieces)
            assert np.array_equal(win.astype(np.float64), wbins), (name, pieces)
            del keep


def ctx_ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("layout", ["samtools", "htsjdk20000"])
def test_unfinished_record_larger_than_a_block_is_carried(ctx, layout):
    """A record of ~240 KB (over four of samtools' blocks): calls that end inside it, and a call in which no record is whole
    (its whole stream is the carried record's), index every record of the file; depth and windows then equal the oracle's."""
    soa = BL.big_record_soa()
    data, bounds = _stream(soa, 4)
    raw = _pack(layout, data, bounds)
    blks, start, first = _block_starts(raw, bounds)
    nb = len(blks) - first
    big = int(np.argmax(np.diff(bounds)))
    assert bounds[big + 1] - bounds[big] > 3 * 65536
    inside = [i - first for i in range(first, len(blks)) if bounds[big] < start[i] and start[i] + blks[i][2] < bounds[big + 1]]
    assert len(inside) >= 2
    k0 = inside[0]
    # ends inside it | + a call that is all inside it | ... two such calls | the rest
    cut_sets = [[0, k0, nb], [0, k0, k0 + 1, nb], [0, k0, k0 + 1, k0 + 2, nb], [0, k0 + 1, nb], [0, k0, inside[-1] + 1, nb]]
    rng = np.random.default_rng(11)
    cut_sets += [[0] + sorted(int(x) for x in rng.choice(np.arange(1, nb), 3, replace=False)) + [nb] for _ in range(4)]
    for cuts in cut_sets:
        _calls(ctx, raw, data, bounds, cuts)
    W = 1000
    tlen = soa.refs[0][1]
    assert ctx.L.hpn_depth_begin(ctx.h, 0, tlen, 0x704) == 0
    keep = _calls(ctx, raw, data, bounds, [0, k0, k0 + 1, nb],
                  each=lambda d: ctx._ck(ctx.L.hpn_depth_add_raw_dev(ctx.h, ctx_ptr(d)), "hpn_depth_add_raw_dev"))
    runs, win = ctx.depth_finish(tlen, W)
    rc, wruns, wbins = orc.depth_target(soa, 0, W, 0x704)
    assert rc == 0 and np.array_equal(runs, wruns) and np.array_equal(win.astype(np.float64), wbins)
    del keep


# ---- what only the raw route has --------------------------------------------------------------------------------------

def test_n_cigar_from_none_to_65535(ctx):
    """n_cigar 0 (mapped), 1 .. 5, 16, 255, 1000, 65535, the last M followed or not by D / N / I / S: RawRecs reads every
    operation in place, and the reach walk (k_depth_index) sees every one."""
    soa = BL.ncigar_soa()
    assert set(np.diff(soa.cigar_off.astype(np.int64)).tolist()) >= set(BL.N_CIGARS)
    _raw_check(ctx, soa, 5, depth=[(1000, 0x704), (20000, 0x4)], window=[1000])


def test_cigar_starts_at_every_offset(ctx):
    """l_read_name 2 .. 255 with aux of every length: the CIGAR starts at every offset mod 16, record heads cross 128-byte lines."""
    soa = make_soa(6000, [("chrA", 800_000)], 61, cigars=["150M", "40M2I108M", "10M3000N140M", "5S100M45S", "60M5D90M"])
    data, bounds = _stream(soa, 61)
    nm = BL.cycling_names(len(soa.tid))
    cig_at = bounds[:-1] + 36 + np.diff(nm[1]) + 1
    assert set((cig_at % 16).tolist()) == set(range(16))
    assert ((bounds[:-1] % 128) > 128 - 36).any() and set((bounds[:-1] % 16).tolist()) == set(range(16))
    _raw_check(ctx, soa, 61, depth=[(1000, 0x704)], window=[1000])


def test_far_gaps_on_the_tile_lattice(ctx):
    soa = BL.lattice_soa()
    _raw_check(ctx, soa, 13, depth=[(1000, 0x704), (20000, 0x4), (1, 0x704)], window=[1000])


def test_long_reads_among_short_ones(ctx):
    """l_seq 257 .. 20,000 (the window kernel's generic path) and SEQ * among 150-base reads in the same waves; three 70,000-base
    all-G reads on chrM whose G/C wraps in the reference's unsigned short (3 x (70,000 mod 65,536) = 13,392 in window 0); an
    odd-length long read last."""
    soa = BL.long_read_soa()
    assert soa.l_qseq[-1] % 2 == 1 and soa.l_qseq[-1] > 20_000
    rc, off, wb, wg, *_ = orc.window_counts(soa, 20000)
    assert rc == 0 and int(wg[0]) >= 3 * (70_000 - 65_536)
    _raw_check(ctx, soa, 21, depth=[(1000, 0x704)], window=[1000, 20000], layouts=LAYOUTS + ("htsjdk20000",))


@pytest.mark.parametrize("block", [97, 1000, 20000])
def test_embedded_record_chains_are_refuted(ctx, block):
    """aux payloads that hold well-formed chains of records with printable names: a block starting inside one finds its first
    'record' there, four in a row; the proof from the call's first record must refute it, not count it."""
    soa = make_soa(8000, [("chrA", 900_000), ("chrB", 300_000)], 71, cigars=["150M", "10S140M", "50M2048N50M"])
    _raw_check(ctx, soa, 71, depth=[(1000, 0x704)], window=[1000], layouts=("htsjdk%d" % block,), aux="chain")
