"""CPU: tests/prim_ref.py -- the reference test_scan_sort_gpu.py holds the device to -- against a hand-written loop and
sorted(..., key=...) on a few dozen items."""
import numpy as np
import pytest

import prim_ref


def loop_scan(values, bits):
    out = [0] * (len(values) + 1)
    for i in range(len(values)):
        out[i + 1] = (out[i] + values[i]) % (1 << bits)
    return out


SCAN_SETS = {
    "empty": [],
    "one": [5],
    "small": [3, 0, 0, 7, 1, 0, 2, 9, 4, 4, 0, 1],
    "passes 2^32": [0xFFFFFFFF, 1, 0xFFFFFFFF, 0xFFFFFFFE, 7, 0, 0xFFFFFFFF, 3] * 5,
    "passes 2^61": [(1 << 59) + 11, 1 << 59, (1 << 60) - 1, 5, (1 << 59) + 3, 0, (1 << 60) + 9, 1],
    "passes 2^64": [(1 << 64) - 1, 1, 0, (1 << 63) + 5, (1 << 64) - 2, 3, 1 << 63, 9] * 4,
}


@pytest.mark.parametrize("what", sorted(SCAN_SETS))
@pytest.mark.parametrize("bits", [32, 64])
def test_excl_scan_against_a_loop(what, bits):
    values = SCAN_SETS[what]
    dtype = np.uint64 if any(v >> 32 for v in values) else np.uint32
    got = prim_ref.excl_scan(np.array(values, dtype), bits)
    assert got.dtype == (np.uint32 if bits == 32 else np.uint64)
    assert got.tolist() == loop_scan(values, bits)


def test_excl_scan_sets_pass_what_they_claim():
    assert sum(SCAN_SETS["passes 2^32"]) > 1 << 32
    assert 1 << 61 < sum(SCAN_SETS["passes 2^61"]) < 1 << 62
    assert sum(SCAN_SETS["passes 2^64"]) > 1 << 66
    assert int(prim_ref.excl_scan(np.array(SCAN_SETS["passes 2^32"], np.uint32), 64)[-1]) == sum(SCAN_SETS["passes 2^32"])
    assert int(prim_ref.excl_scan(np.array(SCAN_SETS["passes 2^32"], np.uint32), 32)[-1]) == sum(SCAN_SETS["passes 2^32"]) % (1 << 32)
    assert int(prim_ref.excl_scan(np.array(SCAN_SETS["passes 2^61"], np.uint64), 64)[-1]) == sum(SCAN_SETS["passes 2^61"])


def pairs(n=48, seed=7):
    """n keys random in all 64 bits, every third one a repeat of an earlier key with a few bits changed, so that every field
    below has ties; payloads with repeats."""
    rs = np.random.RandomState(seed)
    keys = [int(rs.randint(0, 1 << 32)) << 32 | int(rs.randint(0, 1 << 32)) for _ in range(n)]
    for i in range(2, n, 3):
        keys[i] = keys[i - 2] ^ (1 << int(rs.randint(0, 64)))
    vals = [int(v) for v in rs.randint(0, 9, n)]
    return keys, vals


@pytest.mark.parametrize("begin,end", [(0, 64), (0, 1), (4, 12), (13, 37), (0, 12), (63, 64), (5, 5), (64, 64)])
def test_sort_bits_against_sorted(begin, end):
    keys, vals = pairs()
    field = lambda k: (k >> begin) & ((1 << (end - begin)) - 1)
    want = sorted(zip(keys, vals), key=lambda p: field(p[0]))   # (sorted is stable)
    k, v = prim_ref.sort_bits(np.array(keys, np.uint64), np.array(vals, np.uint32), begin, end)
    assert list(zip(k.tolist(), v.tolist())) == want
    assert prim_ref.bit_field(np.array(keys, np.uint64), begin, end).tolist() == [field(x) for x in keys]
    if begin == end:
        assert k.tolist() == keys and v.tolist() == vals


@pytest.mark.parametrize("digits", [0x81, 0x55, 0x01, 0xFF, 0])
def test_sort_digits_against_sorted(digits):
    keys, vals = pairs(seed=11)

    def field(k):
        return sum(k & (0xFF << (8 * d)) for d in range(8) if (digits >> d) & 1)

    want = sorted(zip(keys, vals), key=lambda p: field(p[0]))
    k, v = prim_ref.sort_digits(np.array(keys, np.uint64), np.array(vals, np.uint32), digits)
    assert list(zip(k.tolist(), v.tolist())) == want
    assert prim_ref.digit_field(np.array(keys, np.uint64), digits).tolist() == [field(x) for x in keys]


def test_sort_fields_have_ties_and_differ():
    # the cases above mean something only if the fields tie somewhere and order the keys differently
    keys, vals = pairs()
    k = np.array(keys, np.uint64)
    assert len(set(prim_ref.bit_field(k, 4, 12).tolist())) < len(keys) or len(set(prim_ref.bit_field(k, 0, 1).tolist())) == 2
    a = prim_ref.sort_bits(k, np.array(vals, np.uint32), 4, 12)[0].tolist()
    b = prim_ref.sort_bits(k, np.array(vals, np.uint32), 0, 12)[0].tolist()
    c = prim_ref.sort_bits(k, np.array(vals, np.uint32), 0, 16)[0].tolist()
    assert a != b and b != c
