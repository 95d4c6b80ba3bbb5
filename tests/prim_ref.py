"""Plain references of the two shared primitives (kernels/radix_sort.hpp: k_excl_scan, radix_sort_pairs and
uniq_sort_pairs_digits), pinned on the host by test_prim_ref_host.py and compared exactly with the device by
test_scan_sort_gpu.py."""
import itertools

import numpy as np


def excl_scan(values, out_bits):
    """The n + 1 exclusive prefix sums of `values`, summed with Python integers and reduced modulo 2^out_bits."""
    assert out_bits in (32, 64)
    sums = list(itertools.accumulate(np.asarray(values).tolist(), initial=0))   # (tolist: Python integers, so no sum wraps)
    if sums[-1] >> 64:   # (the sums ascend: none before the last is larger)
        sums = [s & 0xFFFFFFFFFFFFFFFF for s in sums]
    out = np.array(sums, np.uint64)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32) if out_bits == 32 else out


def bit_field(keys, begin, end):
    """(key >> begin) & (2^(end - begin) - 1) of uint64 keys, 0 <= begin <= end <= 64."""
    assert 0 <= begin <= end <= 64
    keys = np.asarray(keys, np.uint64)
    if begin == end:
        return np.zeros(keys.shape, np.uint64)
    width = end - begin
    mask = np.uint64((1 << width) - 1)
    return (keys >> np.uint64(begin)) & mask


def sort_bits(keys, vals, begin, end):
    """(keys, vals) in the stable order of the key bits [begin, end); the keys stay whole."""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    order = np.argsort(bit_field(keys, begin, end), kind="stable")
    return keys[order], vals[order]


def digit_field(keys, digits):
    """The uint64 keys with every byte zeroed whose bit is clear in digits (bit d: key bits [8 d, 8 d + 8))."""
    assert 0 <= digits < 256
    mask = 0
    for d in range(8):
        if (digits >> d) & 1:
            mask |= 0xFF << (8 * d)
    return np.asarray(keys, np.uint64) & np.uint64(mask)


def sort_digits(keys, vals, digits):
    """(keys, vals) in the stable order of the key with the unselected bytes zeroed; the keys stay whole."""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    order = np.argsort(digit_field(keys, digits), kind="stable")
    return keys[order], vals[order]
