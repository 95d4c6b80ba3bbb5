"""Plain numpy / Python restatement of the K2 cut and of the quality-threshold trim points (include/hpngs.h: hpn_fastq_trim,
hpn_fastq_trim_points, hpn_fastq_qtrim_points).  No ctypes: test_trim_ref_host.py holds it against the C oracle, and
test_trim_paths_gpu.py holds the kernels of kernels/fastq_trim.hip against it.  All integers and bytes: every comparison is exact.

A batch is (seq u8[], qual u8[], off u64[n+1]); `off` may be a window of a longer batch (off[0] > 0): record i is the bytes
[off[i], off[i+1]) of the arrays as passed, and the packed output starts at 0.
"""
import numpy as np

WAVE = 64                       # records one wave of k_trim_copy owns
FAST_MIN, FAST_MAX = 16, 1024   # kept counts at which a wave of equal counts takes the fast path


def _points(off, beg, end):
    """Per record the clamped [b, e) of the contract: b = min(beg, len), e = min(end, len), empty when e <= b."""
    o = np.asarray(off, np.uint64).astype(np.int64)
    ln = o[1:] - o[:-1]
    b = np.minimum(np.asarray(beg, np.uint64).astype(np.int64), ln)
    e = np.minimum(np.asarray(end, np.uint64).astype(np.int64), ln)
    return o, b, np.maximum(e, b)


def kept_counts(off, beg, end):
    """Bytes every record keeps (int64[n]); beg / end are scalars (fixed cycles) or one value per record."""
    _, b, e = _points(off, beg, end)
    return e - b


def cut_points(seq, qual, off, beg, end):
    """-> (out_seq, out_qual, out_off): every record cut to its own [min(beg, len), min(end, len)), packed."""
    o, b, e = _points(off, beg, end)
    n = len(o) - 1
    out_off = np.zeros(n + 1, np.uint64)
    np.cumsum(e - b, out=out_off[1:])
    lo, hi = (o[:-1] + b).tolist(), (o[:-1] + e).tolist()
    empty = np.zeros(0, np.uint8)
    out_seq = np.concatenate([empty] + [seq[lo[i]:hi[i]] for i in range(n)])
    out_qual = np.concatenate([empty] + [qual[lo[i]:hi[i]] for i in range(n)])
    return out_seq, out_qual, out_off


def cut(seq, qual, off, S, E):
    """-> (out_seq, out_qual, out_off): the fixed cycles [S, E) of every record (0 <= S <= E)."""
    assert 0 <= S <= E
    return cut_points(seq, qual, off, S, E)


def qtrim_points(qual, off, T):
    """-> (beg, end) uint32[n]: index of the first quality byte >= T, and 1 + index of the last one; 0, 0 when there is none.
    T is an unsigned 32-bit threshold: above 255 nothing can reach it."""
    assert 0 <= T <= 0xFFFFFFFF
    o = np.asarray(off, np.uint64).astype(np.int64).tolist()
    n = len(o) - 1
    beg, end = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i in range(n):
        hit = np.flatnonzero(qual[o[i]:o[i + 1]].astype(np.uint64) >= np.uint64(T))
        if len(hit):
            beg[i], end[i] = hit[0], hit[-1] + 1
    return beg, end


def qtrim_points_flat(qual, off, T):
    """qtrim_points without the loop over records, for the one batch of half a million of them: the flat positions of all hits,
    each with its record; a record's first and last hit are the first and last entry of its run."""
    assert 0 <= T <= 0xFFFFFFFF
    o = np.asarray(off, np.uint64).astype(np.int64)
    n = len(o) - 1
    beg, end = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    hit = o[0] + np.flatnonzero(qual[o[0]:o[n]].astype(np.uint64) >= np.uint64(T))
    rec = np.searchsorted(o, hit, side="right") - 1           # the last record that starts at or before the byte: never an empty one
    if len(hit):
        first = np.flatnonzero(np.concatenate([[True], rec[1:] != rec[:-1]]))
        last = np.concatenate([first[1:], [len(hit)]]) - 1
        beg[rec[first]] = hit[first] - o[rec[first]]
        end[rec[last]] = hit[last] - o[rec[last]] + 1
    return beg, end


def wave_counts(off, beg, end):
    """The kept counts as k_trim_copy's waves see them: int64[waves, 64], wave w = records 64 w .. 64 w + 63 of the batch as
    passed, lanes past the last record keep 0 bytes."""
    c = kept_counts(off, beg, end)
    pad = (-len(c)) % WAVE
    return np.concatenate([c, np.zeros(pad, np.int64)]).reshape(-1, WAVE)


def uniform_waves(off, beg, end, lo=FAST_MIN, hi=FAST_MAX):
    """c0 of every wave that takes the fast path of k_trim_copy, in wave order: the kept count of lane 0 lies in lo..hi and all
    64 kept counts equal it.  (The kernel also wants the wave's sources and destinations within 4 GiB of lane 0's; 64 records
    of any batch a test can build are.)"""
    w = wave_counts(off, beg, end)
    c0 = w[:, 0]
    ok = (c0 >= lo) & (c0 <= hi) & (w == c0[:, None]).all(axis=1)
    return c0[ok].tolist()
