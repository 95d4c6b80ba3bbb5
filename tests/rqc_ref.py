"""Python restatement of the R plugin's qsort_hash_count(fq1, fq2) (Rgzfastq_uniq.c): framing (uniq_ref.records: the four gzgets
of readNextNode), the key the plugin assembles in its zeroed 512-byte buffer, the counts of the distinct keys sorted descending,
the Quality / Nucleotide / Length tallies in the plugin's layouts, the per-read GC fraction (count / L in float64) and the stderr
lines.

Held to the recorded reference runs by test_rqc_golden.py; the GPU tests then use it as the checker.  Where the plugin has no
answer `NoAnswer` is raised with .record, .mate (0, 1) and .reason (the HPN_RFASTQC_* numbers)."""
import collections
import struct

import numpy as np

from uniq_ref import NoAnswer as _NoAnswer
from uniq_ref import records

MAXLEN = 300
BAD_LENGTH, BAD_QUALITY, BAD_BYTE, MATE_SHORT = 1, 2, 3, 4
NT = {ord(c): v for c, v in (("t", 0), ("T", 0), ("u", 0), ("U", 0), ("c", 1), ("C", 1), ("a", 2), ("A", 2), ("g", 3), ("G", 3), (".", 4), ("N", 4))}
NT_LUT = np.array([NT.get(b, 0) for b in range(256)])
STDERR = "mean GC%% = %s%%\nhash size: %d\nunique reads %d (%d/%d= %s%% )\nFinished load hash at T s\nFinished at T s\n"


class NoAnswer(_NoAnswer):
    def __init__(self, what, record=-1, mate=0, reason=0):
        super().__init__(what)
        self.record, self.mate, self.reason = record, mate, reason


def key(s1: bytes, s2: bytes = None) -> bytes:
    """The C string in the plugin's buffer: memcpy of mate 1 (its first 50 bytes when longer than 75), of mate 2 to offset 50 (its
    first 50 bytes when longer than 75) or to offset len(s1), then whatever stands in front of the first NUL."""
    buf = bytearray(512)
    head = s1[:50] if len(s1) > 75 else s1
    buf[:len(head)] = head
    if s2 is not None:
        if len(s2) > 75:
            buf[50:100] = s2[:50]
        else:
            buf[len(s1):len(s1) + len(s2)] = s2
    return bytes(buf[:buf.index(0)])


def first_bad(mates):
    """(2 * record + mate, reason) of the first record the plugin has no answer for, or None.  mates: one or two lists of
    (name, sequence, quality).  In the plugin's order -- per record mate 1, then mate 2 -- with lengths looked at before bytes, as
    hpn_rfastqc_finish does; a mate 2 that runs out is its missing record."""
    n = len(mates[0])
    n_mate = [n] + ([min(n, len(mates[1]))] if len(mates) > 1 else [])
    short = 2 * len(mates[1]) + 1 if len(mates) > 1 and len(mates[1]) < n else None

    def smallest(test):
        keys = [2 * i + m for m, recs in enumerate(mates) for i in range(n_mate[m]) if test(recs[i][1], recs[i][2])]
        return min(keys) if keys else None

    lens = smallest(lambda s, q: not 1 <= len(s) <= MAXLEN or len(q) > MAXLEN)
    if lens is not None and (short is None or lens < short):
        s = mates[lens & 1][lens >> 1][1]
        return lens, BAD_LENGTH if not 1 <= len(s) <= MAXLEN else BAD_QUALITY
    byte = smallest(lambda s, q: max(s + q, default=0) >= 128)
    if short is not None and (byte is None or short < byte):
        return short, MATE_SHORT
    return (byte, BAD_BYTE) if byte is not None else None


class Result:
    pass


def tally(data1: bytes, data2: bytes = None) -> Result:
    mates = [list(records(data1))] + ([list(records(data2))] if data2 is not None else [])
    bad = first_bad(mates)
    if bad is not None:
        raise NoAnswer("record %d of mate %d: reason %d" % (bad[0] >> 1, (bad[0] & 1) + 1, bad[1]), bad[0] >> 1, bad[0] & 1, bad[1])
    n = len(mates[0])
    r = Result()
    r.n = n
    r.gc, r.quality, r.nucleotide, r.length = [], [], [], []
    for recs in mates:
        gc = np.zeros(n, np.float64)
        quality, nucleotide, length = np.zeros(128 * MAXLEN, np.int32), np.zeros(5 * MAXLEN, np.int32), np.zeros(MAXLEN, np.int32)
        for i, (_, s, q) in enumerate(recs[:n]):      # (a longer mate 2: its extra records are never read)
            gc[i] = np.float64(s.count(b"G") + s.count(b"C")) / np.float64(len(s))
            nucleotide[5 * np.arange(len(s)) + NT_LUT[np.frombuffer(s, np.uint8)]] += 1      # (one cell per position: no index twice)
            quality[np.frombuffer(q, np.uint8) + 128 * np.arange(len(q))] += 1
            length[len(s) - 1] += 1
        r.gc.append(gc), r.quality.append(quality), r.nucleotide.append(nucleotide), r.length.append(length)
    counts = collections.Counter(key(mates[0][i][1], mates[1][i][1] if data2 is not None else None) for i in range(n))
    r.keys = counts
    r.dup = np.array(sorted(counts.values(), reverse=True), np.int32)
    return r


def elements(r: Result):
    """The list's elements in the plugin's order."""
    out = [r.dup]
    for m in range(len(r.gc)):
        out += [r.gc[m], r.quality[m], r.nucleotide[m], r.length[m]]
    return out


def table_size(n_unique: int) -> int:
    size = 13400000
    while n_unique and float(n_unique - 1) >= size * 0.75:
        size = 2 * size + 1
    return size


def _pct(x, digits):
    """printf("%f") / ("%.3f") of a double, "-nan" where the plugin divides 0 by 0."""
    return "-nan" if x != x else "%.*f" % (digits, x)


def stderr_text(r: Result) -> str:
    total = 0.0
    for g in r.gc[0]:      # a sequential double sum in input order
        total += float(g)
    with np.errstate(all="ignore"):
        mean = float(np.float64(total) / np.float64(r.n) * 100)
        share = float(np.float64(len(r.dup)) / np.float64(r.n) * 100)
    return STDERR % (_pct(mean, 6), table_size(len(r.dup)), len(r.dup), len(r.dup), r.n, _pct(share, 3))


def raw(a) -> bytes:
    """An element as the little-endian bytes the tool writes and R's readBin reads."""
    return a.astype("<f8" if a.dtype == np.float64 else "<i4").tobytes()


def first_doubles(a, k=8):
    return [struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in a[:k]]
