"""Python restatement of gzfastq_sample's two selection rules and its output format.

Held to the recorded reference outputs by test_sample_golden.py; the GPU tests then use it as the
checker for random inputs.  Works on REGULAR text only (whole records, lines of at most 1022
characters + newline, no NUL byte) -- outside of that the reference crashes.
"""
import ctypes
import math

import numpy as np


class Irregular(ValueError):
    pass


def frame(data: bytes):
    """The records as readNextNode frames them: (name, seq, quality-line-with-its-newline)."""
    if b"\0" in data:
        raise Irregular("NUL byte")
    lines = data.split(b"\n")
    open_end = lines[-1] != b""
    if not open_end:
        lines.pop()
    if len(lines) % 4:
        raise Irregular("stream ends inside a record")
    if any(len(x) > 1022 for x in lines):
        raise Irregular("line of 1023+ characters")
    recs = []
    for i in range(0, len(lines), 4):
        lastq = open_end and i + 4 == len(lines)
        recs.append((lines[i], lines[i + 1], lines[i + 3] + (b"" if lastq else b"\n")))
    return recs


def x31(name: bytes) -> int:
    """khash.h's X31 string hash: bytes as signed chars, 32-bit wrap-around; empty -> 0."""
    h = 0
    for c in name:
        h = (h * 31 + (c - 256 if c >= 128 else c)) & 0xFFFFFFFF
    return h


def threshold(frac: float) -> int:
    """keep iff (k & 0xffffff) / 2^24 < frac  <=>  (k & 0xffffff) < ceil(frac * 2^24)."""
    return max(0, min(1 << 24, math.ceil(frac * (1 << 24))))


def parse_s(arg: str):
    """-s SEED.FRAC -> (seed_add, frac): strtol, srand/rand of the C library when non-zero, strtod of the rest."""
    i = 0
    while i < len(arg) and (arg[i].isdigit() or (i == 0 and arg[i] in "+-")):
        i += 1
    seed = int(arg[:i]) if arg[:i].strip("+-") else 0
    if seed:
        libc = ctypes.CDLL(None)
        libc.srand(ctypes.c_uint(seed & 0xFFFFFFFF))
        seed = libc.rand()
    rest = arg[i:]
    try:
        frac = float(rest) if rest else 0.0
    except ValueError:
        frac = 0.0
    return seed & 0xFFFFFFFF, frac


def keep_fraction(recs, seed_add: int, thr: int):
    return [i for i, r in enumerate(recs) if ((x31(r[0]) + seed_add) & 0xFFFFFF) < thr]


def draw_picks(n: int, pick: int):
    """Fisher-Yates over 0..n-1 driven by MT19937(4357), first `pick` entries, sorted."""
    rs = np.random.RandomState(4357)
    xs = list(range(n))
    buf, at = np.zeros(0, np.uint32), 0
    for i in range(n - 1, 0, -1):
        k = i + 1
        scale = 0xFFFFFFFF // k
        while True:
            if at == len(buf):
                buf, at = np.frombuffer(rs.bytes(4 * 4096), dtype="<u4"), 0
            j = int(buf[at]) // scale
            at += 1
            if j < k:
                break
        xs[i], xs[j] = xs[j], xs[i]
    return sorted(xs[:pick])


def render(recs, kept, fasta=False, first_ordinal=0) -> bytes:
    out = []
    for i in kept:
        name, seq, q = recs[i]
        tag = b"_%d\n" % (first_ordinal + i + 1)
        out.append(b">" + name + tag + seq + b"\n" if fasta else name + tag + seq + b"\n+\n" + q)
    return b"".join(out)


def render_mate(recs2, kept, fasta=False) -> bytes:
    """The -2 file: record i is written exactly when record i of -1 is, as long as the mate file has one."""
    return render(recs2, [i for i in kept if i < len(recs2)], fasta)


def simulate(args, name1, data1, name2=None, data2=None):
    """The whole tool on regular inputs: ({output file name: decompressed bytes, or None for a 0-byte file}, stderr
    with the run times as 'T').  `args` are the command line's arguments besides -1 / -2."""
    fasta, s_arg, n_arg = False, None, 0
    it = iter(args)
    for a in it:
        if a == "-f":
            fasta = True
        elif a == "-q":
            fasta = False
        elif a == "-s":
            s_arg = next(it)
        elif a == "-n":
            n_arg = int(next(it))
        elif a == "-o":
            next(it)
        else:
            raise ValueError(a)
    recs1 = frame(data1)
    recs2 = frame(data2) if data2 is not None else None
    out, err = {}, ""

    def stats(n, k):
        ratio = "-nan" if n == 0 else "%.6f" % (k / n)
        return "total reads: %d\npick out: %d (%d/%d=%s)\n" % (n, k, k, n, ratio)

    if s_arg is not None:
        seed_add, frac = parse_s(s_arg)
        if frac > 0:
            kept = keep_fraction(recs1, seed_add, threshold(frac))
            out["%s.%f.gz" % (name1, frac)] = render(recs1, kept, fasta)
            if recs2 is not None:
                out["%s.%f.gz" % (name2, frac)] = render_mate(recs2, kept, fasta)
            err += stats(len(recs1), len(kept))
    if n_arg:
        n = len(recs1)
        err += "total_reads_num: %d\nFinished count_read at T s\n" % n
        if n_arg > n:
            out["%s.%d.gz" % (name1, n_arg)] = None
            return out, err + "pick_count > read_count (%d > %d)\n" % (n_arg, n)
        kept = draw_picks(n, n_arg)
        out["%s.%d.gz" % (name1, n_arg)] = render(recs1, kept, fasta)
        if recs2 is not None:
            out["%s.%d.gz" % (name2, n_arg)] = render_mate(recs2, kept, fasta)
        err += "Start_read at T s\nEnd_read at T s\n" + stats(n, n_arg)
    return out, err + "Finished at T s\n"
