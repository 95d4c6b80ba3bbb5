"""K1 `k_tally_scan`: byte tiles counted from a line-aligned origin (kOrigin = 128 or 4096 bytes, csrc/kernels/fastq_scan.hip).
The byte range [off[0], off[n]) of a device-resident quality array is moved over every interesting start modulo 4096 and every
interesting end relative to a tile (T = 256 U 16 bytes) and a chunk (8 T), in the coordinates of the origin under test, plus ranges
too short to hold a whole 16-byte vector.  Every byte outside the range is 0xFF, which reports E_DOMAIN if a mask lets it through;
one 0xFF inside, at the first or the last byte, must report it.  Bit-exact against the C oracle (count_soa) on the window alone.

Runs on the shipped library, on the test-hooks library with both origins at variant 811 (HPN_K1_VARIANT=811@128 / 811@4096), and at
the shipped origin with the other unrolls and schedules."""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

SHIPPED_ORIGIN = 128        # kK1Origin
RUNS = [None, "811@128", "811@4096", "810", "812", "411", "1611"]      # None: the shipped library
STARTS = (0, 1, 15, 16, 17, 111, 112, 113, 127, 128, 129, 4095)        # (data_ptr + b0) mod 4096
END_TILES, END_DELTAS = (1, 8, 17), (-17, -16, -1, 0, 1, 16, 17)       # the end at k T + d from the origin
TINY = (0, 1, 14, 15, 16, 17, 31, 32, 33)                              # nbytes: inside one vector, no whole vector, exactly one
PLANTED = (0, 52, 53, 62, 63, 127)                                     # both sides of the two thresholds and of the domain


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def _geometry(run):
    variant, _, origin = (run or "811").partition("@")
    return int(variant) // 100, int(origin) if origin else SHIPPED_ORIGIN


def _offsets(cum, nbytes):
    """Ragged records of 1..300 bytes that fill [0, nbytes): a prefix of the drawn lengths and one record for what is left."""
    if nbytes == 0:
        return np.zeros(1, np.uint64)
    k = int(np.searchsorted(cum, nbytes, side="right"))
    off = np.concatenate([[0], cum[:k]]).astype(np.uint64)
    return off if int(off[-1]) == nbytes else np.concatenate([off, [nbytes]]).astype(np.uint64)


class Bench:
    """The quality bytes on host and device and one launch of a window [b0, b0 + nbytes) of them."""

    def __init__(self, ctx, U):
        import torch
        self.torch, self.ctx = torch, ctx
        self.T = 256 * U * 16
        size = max(END_TILES) * self.T + max(END_DELTAS) + 4096 + 64
        rng = np.random.default_rng(950 + U)
        self.qual = rng.integers(0, 128, size, dtype=np.uint8)
        plant = rng.random(size) < 0.3
        self.qual[plant] = rng.choice(np.array(PLANTED, np.uint8), int(plant.sum()))
        self.cum = np.cumsum(rng.integers(1, 301, size // 100))       # ~150 bytes per record: more than enough to fill the array
        self.d_qual = torch.from_numpy(self.qual).cuda()
        self.d_win = torch.empty_like(self.d_qual)
        self.ptr = self.d_win.data_ptr()

    def start(self, residue):
        return (residue - self.ptr) % 4096

    def run(self, b0, nbytes, poison=None):
        torch = self.torch
        assert 0 <= b0 and b0 + nbytes + 16 <= self.qual.size
        off = _offsets(self.cum, nbytes)
        self.d_win.fill_(0xFF)
        self.d_win[b0:b0 + nbytes] = self.d_qual[b0:b0 + nbytes]
        if poison is not None:
            self.d_win[b0 + poison] = 0xFF
        d_off = torch.from_numpy((off + np.uint64(b0)).astype(np.int64)).cuda()
        self.ctx.fastq_tally_dev(self.d_win, d_off, len(off) - 1)
        got = self.ctx.fastq_tally_fetch()          # raises E_DOMAIN if a byte with bit 7 set was counted
        return got, off

    def check(self, b0, nbytes, what):
        got, off = self.run(b0, nbytes)
        rc, want = orc.count_soa(self.qual[b0:b0 + nbytes].copy(), off)
        assert rc == 0
        s = want.summary()
        assert int(off[-1]) == nbytes == s.sum, what
        assert np.array_equal(got.seqlen, want.seqlen), what + ": seqlen"
        assert (got.total, got.q20, got.q30) == (s.sum, s.q20, s.q30), what + f": total/q20/q30 {(got.total, got.q20, got.q30)} != {(s.sum, s.q20, s.q30)}"


@pytest.mark.parametrize("run", RUNS, ids=lambda r: r or "shipped")
def test_every_start_and_end(request, run):
    from conftest import in_hooks_build
    if run is not None and in_hooks_build(request, {"HPN_K1_VARIANT": run}):
        return
    U, origin = _geometry(run)
    b = Bench(request.getfixturevalue("ctx"), U)
    for residue in STARTS:
        b0 = b.start(residue)
        a = (b.ptr + b0) % origin
        for k in END_TILES:
            for d in END_DELTAS:
                b.check(b0, k * b.T + d - a, f"{run}: start {residue} mod 4096, end {k} T {d:+d}")
        for nbytes in TINY:
            b.check(b0, nbytes, f"{run}: start {residue} mod 4096, {nbytes} bytes")


def test_unknown_origin_is_an_error(request):
    """An origin no kernel was compiled for comes back as an error from the launch, like an unknown variant."""
    from conftest import in_hooks_build
    if in_hooks_build(request, {"HPN_K1_VARIANT": "811@256"}):
        return
    import highperformancengs_amd as hp
    from highperformancengs_amd import _lib
    ctx = request.getfixturevalue("ctx")
    with pytest.raises(hp.HpnError) as e:
        ctx.fastq_tally(np.full(3600, 40, np.uint8), np.arange(0, 3601, 36, dtype=np.uint64))
    assert e.value.status == _lib.E_HIP


@pytest.mark.parametrize("run", RUNS[:3], ids=lambda r: r or "shipped")
def test_a_bad_byte_at_either_end_is_seen(request, run):
    """The masks are not too wide either: 0xFF as the first and as the last byte of the range reports E_DOMAIN, whether that
    byte lies in a partial vector (head, tail, the range inside one vector) or in a whole one of the first and last tile."""
    from conftest import in_hooks_build
    if run is not None and in_hooks_build(request, {"HPN_K1_VARIANT": run}):
        return
    import highperformancengs_amd as hp
    from highperformancengs_amd import _lib
    U, origin = _geometry(run)
    b = Bench(request.getfixturevalue("ctx"), U)
    for residue, end in ((113, (1, -17)), (0, (1, 0)), (4095, (8, 1)), (1, 14), (17, 1), (16, 16), (15, 33)):
        b0 = b.start(residue)
        nbytes = end if isinstance(end, int) else end[0] * b.T + end[1] - (b.ptr + b0) % origin
        for poison in sorted({0, nbytes - 1}):
            with pytest.raises(hp.HpnError) as e:
                b.run(b0, nbytes, poison=poison)
            assert e.value.status == _lib.E_DOMAIN, f"{run}: start {residue} mod 4096, {nbytes} bytes, 0xFF at byte {poison}"
        b.check(b0, nbytes, f"{run}: start {residue} mod 4096, {nbytes} bytes, after the bad byte")
