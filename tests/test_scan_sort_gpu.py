"""GPU: the two primitives under every store-backed tool on their own -- hpn_excl_scan (k_excl_scan through uniq_scan32, uniq_scan64
and uniq_scan64w) and hpn_sort_pairs_u64_bits / _digits (radix_sort_pairs, uniq_sort_pairs_digits) -- against tests/prim_ref.py,
which test_prim_ref_host.py pins on the host.  Every comparison is exact.

The geometry the sizes sit on (kernels/radix_sort.hpp; restated here, the header is not read): the scan gives a lane 8 items
(kScanItems), a wave 512 and a workgroup 2048 -- one tile, kScanThreads = 256 -- and a tile's look-back inspects 64 earlier
tiles at a time, so only from 65 tiles on is there a second window.  The sort gives a wave 64 keys per round and 32 rounds, 2048
keys -- one tile, kSortTile -- and a workgroup four waves, 8192 keys (kSortThreads = 256)."""
import numpy as np
import pytest

import prim_ref

pytestmark = pytest.mark.gpu

SCAN_LANE, SCAN_WAVE, SCAN_TILE, LOOKBACK = 8, 512, 2048, 64
SORT_ROUND, SORT_TILE, SORT_GROUP = 64, 2048, 8192

WIDTHS = [(32, 32), (32, 64), (64, 64)]
SCAN_SIZES = [0, 1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 64 * 2048 - 1, 64 * 2048, 64 * 2048 + 1, 65 * 2048 + 5,
              130 * 2048 + 3, 300 * 2048 + 77]
ONE_AT = [0, 7, 8, 511, 512, 2047, 2048, -1]   # (-1: n - 1)
SORT_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 1, 70_001]
RANGE_SIZES = [2, 65, 2049, 8193, 70_001]
BIT_RANGES = [(0, 64), (0, 8), (8, 16), (56, 64), (0, 1), (63, 64), (0, 12), (4, 12), (3, 64), (13, 37), (0, 33), (5, 5)]
DIGIT_MASKS = [0x01, 0x80, 0x07, 0x81, 0x55, 0xAA, 0xFF, 0]   # 1, 1, 3, 2, 4, 4, 8 and 0 passes


def test_the_geometry_is_what_the_sizes_assume():
    assert (SCAN_WAVE, SCAN_TILE) == (64 * SCAN_LANE, 256 * SCAN_LANE) and (SORT_TILE, SORT_GROUP) == (32 * SORT_ROUND, 4 * 32 * SORT_ROUND)
    for seam in (SCAN_LANE, SCAN_WAVE, SCAN_TILE, 2 * SCAN_TILE, LOOKBACK * SCAN_TILE):
        assert {seam - 1, seam, seam + 1} <= set(SCAN_SIZES)
    assert sum(n // SCAN_TILE + 1 > LOOKBACK + 1 for n in SCAN_SIZES) >= 3     # tiles that need a second window
    assert max(SCAN_SIZES) // SCAN_TILE + 1 > 4 * LOOKBACK + 1                   # ... and a fifth
    for seam in (SORT_ROUND, 2 * SORT_ROUND, SORT_TILE, SORT_GROUP):
        assert {seam - 1, seam, seam + 1} <= set(SORT_SIZES)


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at {i} of {got.size}: got {int(got[i])}, expected {int(want[i])}")


# ---- the scan -------------------------------------------------------------------------------------------------------------

def full_width(rs, n, bits):
    lo = rs.randint(0, 1 << 32, n, dtype=np.uint64)
    return lo.astype(np.uint32) if bits == 32 else (rs.randint(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32)) | lo


def fixed_sets(n):
    """The value sets that do not depend on a seed, as uint32."""
    sets = {"ones": np.ones(n, np.uint32), "zeros": np.zeros(n, np.uint32)}
    for at in ONE_AT:
        at = n - 1 if at < 0 else at
        if 0 <= at < n and f"one at {at}" not in sets:
            v = np.zeros(n, np.uint32)
            v[at] = 1
            sets[f"one at {at}"] = v
    return sets


def random_sets(n, in_bits, seed):
    """[0, 3) and the widest values the width pair is defined on: all 32 bits of a 32-bit item (a 32-bit sum wraps, the
    reference reduces modulo 2^32), and below 2^40 for 64-bit items, whose total must stay below 2^62."""
    rs = np.random.RandomState(seed)
    small = rs.randint(0, 3, n).astype(np.uint32 if in_bits == 32 else np.uint64)
    wide = full_width(rs, n, 32) if in_bits == 32 else full_width(rs, n, 64) & np.uint64((1 << 40) - 1)
    return {"random in [0, 3)": small, "random, wide": wide}


_fixed_ref = {}   # the fixed sets' sums of the size at hand as uint64 (none passes 2^32): shared by the three width pairs


def fixed_ref(n):
    if _fixed_ref.get("n") != n:
        _fixed_ref.clear()
        _fixed_ref.update(n=n, sums={what: prim_ref.excl_scan(v, 64) for what, v in fixed_sets(n).items()})
    return _fixed_ref["sums"]


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: f"{w[0]}to{w[1]}")
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_against_python_integers(ctx, n, widths):
    in_bits, out_bits = widths
    in_t, out_t = (np.uint32 if in_bits == 32 else np.uint64), (np.uint32 if out_bits == 32 else np.uint64)
    runs = 3 if n // SCAN_TILE + 1 > LOOKBACK else 1   # which window a tile ends up using is the scheduler's: the sums may not depend on it
    want = fixed_ref(n)
    assert all(int(w[-1]) < 1 << 32 for w in want.values())
    for run in range(runs):
        for what, v in fixed_sets(n).items():
            got = ctx.excl_scan(v.astype(in_t), out_bits)
            assert got.size == n + 1
            same(got, want[what].astype(out_t), f"{what}, run {run}")
        if n:
            ones = ctx.excl_scan(np.ones(n, in_t), out_bits)
            same(ones, np.arange(n + 1, dtype=out_t), f"out[i] == i, run {run}")
        for what, v in random_sets(n, in_bits, 1000 * run + n % 997 + in_bits).items():
            assert v.dtype == in_t
            same(ctx.excl_scan(v, out_bits), prim_ref.excl_scan(v, out_bits), f"{what}, run {run}")


def test_scan_32_to_64_passes_4_gib_inside_the_first_tile(ctx):
    n = (1 << 18) + 3
    v = np.full(n, 0xFFFFFFFF, np.uint32)
    want = prim_ref.excl_scan(v, 64)
    assert int(want[2]) > 1 << 32 and int(want[-1]) == n * 0xFFFFFFFF and int(want[-1]) > 1 << 49
    same(ctx.excl_scan(v, 64), want, "all 0xFFFFFFFF")
    same(ctx.excl_scan(v, 32), prim_ref.excl_scan(v, 32), "all 0xFFFFFFFF, modulo 2^32")


def test_scan_64_total_is_the_largest_the_look_back_carries(ctx):
    """The total is exactly 2^62 - 1: a tile hands its sums on in 62 bits, so that is the scan's limit (its precondition)."""
    n = 65 * SCAN_TILE + 5
    rs = np.random.RandomState(62)
    v = [int(x) for x in rs.randint(0, (1 << 62) // (2 * n), n, dtype=np.uint64)]
    rest = (1 << 62) - 1 - sum(v)
    assert rest > 1 << 60
    v[3] += rest // 2               # every tile's prefix is large from the first tile on ...
    v[n // 2] += rest - rest // 2   # ... and one tile's aggregate is
    v = np.array(v, np.uint64)
    want = prim_ref.excl_scan(v, 64)
    assert int(want[-1]) == (1 << 62) - 1
    same(ctx.excl_scan(v, 64), want, "total 2^62 - 1")


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: f"{w[0]}to{w[1]}")
def test_status_reuse(ctx, widths):
    """One context's look-back words from call to call: a longer call's prefix flags must not reach a shorter one, nor the
    reverse."""
    in_bits, out_bits = widths
    for k, n in enumerate([300 * 2048 + 77, 2049, 0, 130 * 2048 + 3]):
        rs = np.random.RandomState(40 + k)
        v = rs.randint(1, 1000, n).astype(np.uint32 if in_bits == 32 else np.uint64)
        same(ctx.excl_scan(v, out_bits), prim_ref.excl_scan(v, out_bits), f"call {k}, n = {n}")


def test_scan_argument_errors(ctx):
    from highperformancengs_amd import _lib
    from highperformancengs_amd.api import _ptr
    v, out = np.ones(16, np.uint64), np.zeros(17, np.uint64)
    scan = lambda i, ib, o, ob, n: ctx.L.hpn_excl_scan(ctx.h, _ptr(i), ib, _ptr(o), ob, n)
    assert scan(v, 64, out, 32, 16) == _lib.E_ARG
    assert scan(v, 16, out, 32, 16) == _lib.E_ARG
    assert scan(None, 32, out, 32, 16) == _lib.E_ARG
    assert scan(v, 32, out, 32, 1 << 31) == _lib.E_DOMAIN
    assert not out.any()
    assert scan(None, 32, out, 64, 0) == _lib.OK and out[0] == 0   # n = 0 takes no input


# ---- the sort -------------------------------------------------------------------------------------------------------------

def payloads(n):
    return {"arange": np.arange(n, dtype=np.uint32), "random with repeats": np.random.RandomState(n % 991).randint(0, max(n // 4, 2), n).astype(np.uint32)}


def upper_bytes(rs, n):
    """Bytes 1 .. 7 of n keys, drawn from n / 3 random values: every pass has work, and keys tie."""
    pool = full_width(rs, max(n // 3, 1), 64) & ~np.uint64(0xFF)
    return pool[rs.randint(0, pool.size, n)]


def key_sets(n):
    """Keys whose low byte -- the first pass's digit, met in the given order -- puts a round of 64 lanes in a given state."""
    rs = np.random.RandomState(n % 983)
    i = np.arange(n, dtype=np.uint64)
    up = upper_bytes(rs, n)
    rand = full_width(rs, n, 64)
    return {"a round shares one digit": up | ((i // np.uint64(64)) % np.uint64(256)),
            "digit = lane": up | (i % np.uint64(64)),
            "digits alternate 0 and 255": up | ((i % np.uint64(2)) * np.uint64(255)),
            "digit 0 everywhere": up,   # (at 65 and 2049 the ragged round's dead lanes carry d == 0 too: they are no peers)
            "ascending": np.sort(rand),
            "descending": np.sort(rand)[::-1].copy(),
            "all equal": np.full(n, 0xDEADBEEFCAFEF00D, np.uint64)}


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_all_64_bits(ctx, n):
    for pw, vals in payloads(n).items():
        for kw, keys in key_sets(n).items():
            want_k, want_v = prim_ref.sort_bits(keys, vals, 0, 64)
            for how, (k, v) in {"sort_pairs": ctx.sort_pairs(keys, vals), "bits (0, 64)": ctx.sort_pairs_bits(keys, vals, 0, 64)}.items():
                same(k, want_k, f"keys: {kw}, {pw}, {how}")
                same(v, want_v, f"payload: {kw}, {pw}, {how}")


@pytest.mark.parametrize("bits", BIT_RANGES, ids=lambda b: f"{b[0]}-{b[1]}")
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_sort_bit_range(ctx, n, bits):
    """The stable order of (key >> begin) & mask and of nothing else: keys random in all 64 bits differ above end_bit and
    below begin_bit.  The keys come back whole."""
    begin, end = bits
    keys = full_width(np.random.RandomState(n % 977 + 64 * begin + end), n, 64)
    for pw, vals in payloads(n).items():
        k, v = ctx.sort_pairs_bits(keys, vals, begin, end)
        want_k, want_v = (keys, vals) if begin == end else prim_ref.sort_bits(keys, vals, begin, end)
        same(k, want_k, f"keys, {pw}")
        same(v, want_v, f"payload, {pw}")


@pytest.mark.parametrize("digits", DIGIT_MASKS, ids=lambda d: f"0x{d:02x}")
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_sort_digits(ctx, n, digits):
    """The stable order of the key with the unselected bytes zeroed; an odd number of passes ends in the copy back."""
    keys = full_width(np.random.RandomState(n % 971 + digits), n, 64)
    if n > 1000:   # (ties in the selected bytes too, whatever the mask)
        keys[n // 2:] = keys[:n - n // 2]
    for pw, vals in payloads(n).items():
        k, v = ctx.sort_pairs_digits(keys, vals, digits)
        want_k, want_v = (keys, vals) if digits == 0 else prim_ref.sort_digits(keys, vals, digits)
        same(k, want_k, f"keys, {pw}")
        same(v, want_v, f"payload, {pw}")


def test_sort_argument_errors(ctx):
    from highperformancengs_amd import _lib
    from highperformancengs_amd.api import _ptr
    keys, vals = np.arange(8, 0, -1).astype(np.uint64), np.arange(8, dtype=np.uint32)
    k, v = keys.copy(), vals.copy()
    bits = lambda b, e: ctx.L.hpn_sort_pairs_u64_bits(ctx.h, _ptr(k), _ptr(v), 8, b, e)
    assert bits(9, 8) == _lib.E_ARG
    assert bits(0, 65) == _lib.E_ARG
    assert bits(-1, 8) == _lib.E_ARG
    assert ctx.L.hpn_sort_pairs_u64_digits(ctx.h, _ptr(k), _ptr(v), 8, 256) == _lib.E_ARG
    assert ctx.L.hpn_sort_pairs_u64_bits(ctx.h, None, _ptr(v), 8, 0, 64) == _lib.E_ARG
    assert ctx.L.hpn_sort_pairs_u64_digits(ctx.h, _ptr(k), None, 8, 1) == _lib.E_ARG
    assert ctx.L.hpn_sort_pairs_u64_bits(ctx.h, _ptr(k), _ptr(v), 1 << 31, 0, 64) == _lib.E_DOMAIN
    assert ctx.L.hpn_sort_pairs_u64_digits(ctx.h, _ptr(k), _ptr(v), 1 << 31, 1) == _lib.E_DOMAIN
    assert np.array_equal(k, keys) and np.array_equal(v, vals)


def test_primitives_refuse_while_a_uniq_session_collects(ctx):
    import highperformancengs_amd as hp
    from highperformancengs_amd import _lib
    keys, vals = np.arange(8, 0, -1).astype(np.uint64), np.arange(8, dtype=np.uint32)
    ctx.uniq_begin()
    ctx.uniq_add(b"@a\nACGT\n+\nIIII\n", last=False)
    for call in (lambda: ctx.sort_pairs(keys, vals), lambda: ctx.sort_pairs_bits(keys, vals, 0, 8), lambda: ctx.sort_pairs_digits(keys, vals, 1),
                 lambda: ctx.excl_scan(vals)):
        with pytest.raises(hp.HpnError) as e:
            call()
        assert e.value.status == _lib.E_STATE
    ctx.uniq_add(b"@b\nACGT\n+\nIIII\n", last=True)
    res = ctx.uniq_finish()
    assert (res.n_records, res.n_unique) == (2, 1)   # the session went on undisturbed, and its finished work space is free again
    k, v = ctx.sort_pairs_bits(keys, vals, 0, 8)
    assert k.tolist() == sorted(keys.tolist()) and v.tolist() == vals[::-1].tolist()
    assert ctx.excl_scan(vals).tolist() == [0, 0, 1, 3, 6, 10, 15, 21, 28]
