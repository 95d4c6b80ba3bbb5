"""K1L `k_tally_hist`, the one-length path (stream_uniform), at every read length, count edge and symbol, in all four modes of the
tally: fast (K1), qual_hist, qual_hist + nuc_hist, and nuc_hist alone (the nucleotide-only launch beside K1).

References: the C oracle (count_soa; rqc_soa for the nucleotide matrix of reads of 1..300) and its numpy restatement beyond
(tally_ref.py, held against the oracle in test_tally_ref_host.py).  All integers: every comparison is bit-exact.
"""
import numpy as np
import pytest

from tally_ref import HIST_RECS, LEN_BINS, NUC_LUT, Want, counts_for

pytestmark = pytest.mark.gpu

MODES = ((False, False), (True, False), (True, True), (False, True))     # (qual_hist, nuc_hist); flags = qual_hist + 2 * nuc_hist


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.asarray(got) != np.asarray(want))
        first = tuple(int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} cells differ, first at {first}: got {got[first]}, want {want[first]}; "
                             f"rows {sorted(set(int(b[0]) for b in bad))[:8]}, last at {tuple(int(x) for x in bad[-1])}")


def _compare(got, want, qh, nh, what):
    what = f"{what} qual_hist={qh} nuc_hist={nh}"
    _same(got.seqlen, want.seqlen, what + " seqlen")
    assert (got.total, got.q20, got.q30) == (want.total, want.q20, want.q30), what + " total/q20/q30"
    if qh:
        _same(got.qual_hist, want.qual_hist, what + " qual_hist")
    if nh:
        _same(got.nuc_hist, want.nuc_hist, what + " nuc_hist")


def _check_all(ctx, qual, base, off, what="", want=None):
    """The four modes on a host batch against the references."""
    want = want or Want(qual, base, off)
    for qh, nh in MODES:
        got = ctx.fastq_tally(qual, off, base=base if nh else None, qual_hist=qh, nuc_hist=nh)
        _compare(got, want, qh, nh, what)
    return want


def _check_all_dev(ctx, dq, db, do, n, want, what=""):
    """The four modes on a device-resident batch (do: the offsets from the batch's first record on)."""
    for qh, nh in MODES:
        ctx.fastq_tally_dev(dq, do, n, d_base=db, flags=int(qh) + 2 * int(nh))
        got = ctx.fastq_tally_fetch(qual_hist=qh, nuc_hist=nh)        # raises E_DOMAIN if the kernels flagged the batch
        _compare(got, want, qh, nh, what)


def _random(rng, nbytes):
    return rng.integers(0, 128, max(nbytes, 1), dtype=np.uint8)[:nbytes], rng.integers(0, 256, max(nbytes, 1), dtype=np.uint8)[:nbytes]


def _offsets(lens, lead=0):
    return (lead + np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))])).astype(np.uint64)


# ---- a. every length ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ngr", range(2, 33))
def test_every_length(ctx, ngr):
    """Every read length 16..256 (ngr = groups of 8 cycles per read, the lengths 8 ngr - 7 .. 8 ngr), each at the read counts of
    tally_ref.counts_for; qualities over 0..127, bases over all byte values."""
    rng = np.random.default_rng(1000 + ngr)
    for L in range(max(16, 8 * ngr - 7), 8 * ngr + 1):
        for n in counts_for(L):
            qual, base = _random(rng, n * L)
            _check_all(ctx, qual, base, _offsets(np.full(n, L)), f"L={L} n={n}")


# ---- b. constant symbols and the pour cadence -----------------------------------------------------------------------------------
CONST_LENGTHS = (16, 17, 64, 100, 120, 121, 150, 151, 250, 256)
CONST_QUALS, CONST_BASES = (0, 53, 127), b"TCAGN.X"


@pytest.mark.parametrize("big", ["1", "4", "64"])
def test_constant_symbols(request, big):
    """One quality value and one base in the whole batch: a lane's packed 6-bit counter of that base climbs to the 56 it may hold
    between two pours, and a whole wave's LDS adds fall on one row.  n = `big` chunks in one turn, one chunk more and 17 reads:
    with 64 chunks of 16-byte reads a lane sees 512 items of one symbol and pours nine times.  Every quality value meets every
    base over the lengths; the batches live on the device (the largest is 68 MB per array)."""
    from conftest import in_hooks_build
    if in_hooks_build(request, {"HPN_K1L_BIG": big}):     # (the switch lives in the test-hooks library: host/knobs.hpp)
        return
    import torch
    ctx = request.getfixturevalue("ctx")
    n = HIST_RECS * int(big) + HIST_RECS + 17
    for il, L in enumerate(CONST_LENGTHS):
        off = _offsets(np.full(n, L))
        do = torch.from_numpy(off.astype(np.int64)).cuda()
        for ib, b in enumerate(CONST_BASES):
            q = CONST_QUALS[(ib + il) % len(CONST_QUALS)]
            qual, base = np.full(n * L, q, np.uint8), np.full(n * L, b, np.uint8)
            want = Want(qual, base, off)
            # the closed form: every read adds one count of its symbol at every cycle below L
            code = int(NUC_LUT[b])
            for mat, row in ((want.nuc_hist, code), (want.qual_hist, q)):
                assert (mat[row, :L] == n).all() and int(mat.sum()) == n * L
            dq = torch.full((n * L,), q, dtype=torch.uint8, device="cuda")
            db = torch.full((n * L,), b, dtype=torch.uint8, device="cuda")
            _check_all_dev(ctx, dq, db, do, n, want, f"big={big} L={L} q={q} base={chr(b)!r}")


# ---- c. a one-length chunk followed by 0..8 bytes -------------------------------------------------------------------------------
@pytest.mark.parametrize("L", list(range(17, 24)) + list(range(121, 128)))
def test_one_length_chunk_then_a_few_bytes(ctx, L):
    """4096 reads of L, then one record of t = 0..8 bytes: the chunk's last, partial item is loaded whole when its eight bytes lie
    inside the batch and walked byte by byte when they do not; L % 8 = 1..7 on both sides of the 120 / 121 switch."""
    rng = np.random.default_rng(2000 + L)
    for t in range(9):
        off = _offsets([L] * HIST_RECS + [t])
        qual, base = _random(rng, int(off[-1]))
        _check_all(ctx, qual, base, off, f"L={L} tail={t}")


# ---- d. windows of device-resident data with hostile neighbours -----------------------------------------------------------------
WINDOWS = ((0, 1), (1, 0), (1, 1), (2, 3), (7, 16), (17, 5))       # (records cut off in front, records cut off behind)
N_WINDOW = HIST_RECS + 600


@pytest.mark.parametrize("lo_len,hi_len", [(17, 17), (100, 100), (121, 121), (150, 150), (151, 151), (256, 256), (1, 300), (200, 511)])
def test_windows_with_hostile_neighbours(ctx, lo_len, hi_len):
    """A batch may be a window [off[lo], off[hi]) of larger device arrays.  Every byte outside it is 0xFF in the quality array (no
    row: E_DOMAIN if it reached `seen`) and 'G' in the base array (a count in row 3 if it were tallied); the windows put the first
    byte on several alignments mod 16 and the offsets' pointer on both parities."""
    import torch
    rng = np.random.default_rng(3000 + lo_len + hi_len)
    N = N_WINDOW
    off = _offsets(rng.integers(lo_len, hi_len + 1, N))
    qual0, base0 = _random(rng, int(off[-1]))
    do = torch.from_numpy(off.astype(np.int64)).cuda()
    for cut_lo, cut_hi in WINDOWS:
        lo, hi = cut_lo, N - cut_hi
        w0, w1 = int(off[lo]), int(off[hi])
        qual, base = np.full_like(qual0, 0xFF), np.full_like(base0, ord("G"))
        qual[w0:w1], base[w0:w1] = qual0[w0:w1], base0[w0:w1]
        # the reference sees the host copy of the window alone
        want = Want(qual[w0:w1].copy(), base[w0:w1].copy(), off[lo:hi + 1] - np.uint64(w0))
        dq, db = torch.from_numpy(qual).cuda(), torch.from_numpy(base).cuda()
        _check_all_dev(ctx, dq, db, do[lo:], hi - lo, want, f"len {lo_len}..{hi_len} window ({cut_lo}, {cut_hi})")


# ---- e. the nucleotide-only launch's domain -------------------------------------------------------------------------------------
def test_nucleotide_only_domain(ctx):
    """nuc_hist without qual_hist runs k_tally_hist<false, true> beside K1: the batch's domain is still the quality tally's."""
    import highperformancengs_amd as hp
    from highperformancengs_amd import _lib
    qual, base = np.full(2000, 40, np.uint8), np.full(2000, ord("A"), np.uint8)
    with pytest.raises(hp.HpnError) as e:        # a read of length 512
        ctx.fastq_tally(qual, np.array([0, 100, 612, 700], np.uint64), base=base, nuc_hist=True)
    assert e.value.status == _lib.E_DOMAIN
    q2 = qual.copy()
    q2[777] = 200
    off = np.arange(0, 2001, 100, dtype=np.uint64)
    with pytest.raises(hp.HpnError) as e:        # a quality byte >= 128
        ctx.fastq_tally(q2, off, base=base, nuc_hist=True)
    assert e.value.status == _lib.E_DOMAIN
    # the context is clean afterwards
    got = ctx.fastq_tally(qual, off, base=base, nuc_hist=True)
    assert got.total == 2000 and got.seqlen[100] == 20
    assert (got.nuc_hist[2, :100] == 20).all() and int(got.nuc_hist.sum()) == 2000


@pytest.mark.parametrize("L", [30, 100, 150, 400])
def test_bases_have_no_domain(ctx, L):
    """Bases of 0xFF with sound qualities: no mode raises, every base lands in row 0 (ragged path, both rotations, global cycles)."""
    rng = np.random.default_rng(L)
    n = 1000
    off = _offsets(np.full(n, L) if L != 30 else rng.integers(1, 60, n))
    qual = rng.integers(0, 128, int(off[-1]), dtype=np.uint8)
    base = np.full(int(off[-1]), 0xFF, np.uint8)
    want = _check_all(ctx, qual, base, off, f"L={L} bases 0xFF")
    assert want.nuc_hist.shape == (5, LEN_BINS) and int(want.nuc_hist[0].sum()) == int(off[-1]) and not want.nuc_hist[1:].any()
