"""Inputs of the R plugin's recorded reference runs (tests/golden/make_golden_rqc.py) and of the tests that replay them: FASTQ text
made from fixed seeds and fixed patterns, never stored -- the manifest holds their SHA-256.  A case is (mate 1's text, mate 2's
text or None).

What the shapes are for (the plugin's key: s1[0:50] if L1 > 75 else s1; mate 2 to offset 50 if L2 > 75, else to offset L1):
every length and every pair of lengths comes as a base record, an exact duplicate under another name and quality, and twins that
differ from the base in ONE byte -- at 0, 49, 50 and the last position of mate 1 and of mate 2 -- so that every byte the key sees
and every byte it does not decides a grouping."""
import hashlib
import os

import numpy as np

SE_LENGTHS = [1, 49, 50, 51, 74, 75, 76, 77, 100, 150, 299, 300]
PE_LENGTHS = [1, 49, 50, 51, 75, 76, 100]
TILE = 2048      # kScanTile and kSortTile of radix_sort.hpp (test_rqc_gpu.py checks both)


def seq(rs, n):
    return bytes(rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def qual(rs, n):
    return bytes(rs.randint(33, 74, n).astype(np.uint8).tobytes())


def fq(reads, tag=b"r", eol=b"\n"):
    """reads: (sequence, quality line)."""
    return b"".join(b"@" + tag + b"%d" % i + eol + s + eol + b"+" + eol + q + eol for i, (s, q) in enumerate(reads))


def flip(s, at):
    return s[:at] + (b"A" if s[at:at + 1] != b"A" else b"C") + s[at + 1:]


def twins(L):
    """The positions where a twin differs from its base."""
    return sorted({p for p in (0, 49, 50, L - 1) if 0 <= p < L})


def single_shape(rs, L):
    base = seq(rs, L)
    reads = [base, base] + [flip(base, p) for p in twins(L)]
    return fq([(s, qual(rs, L)) for s in reads])


def pair_shape(rs, L1, L2):
    b1, b2 = seq(rs, L1), seq(rs, L2)
    pairs = [(b1, b2), (b1, b2)] + [(flip(b1, p), b2) for p in twins(L1)] + [(b1, flip(b2, p)) for p in twins(L2)]
    return fq([(a, qual(rs, L1)) for a, _ in pairs], b"p"), fq([(b, qual(rs, L2)) for _, b in pairs], b"p")


def skewed(rs, n, lengths, paired):
    """n records over a pool of keys drawn with a heavy tail: a few keys hundreds of times, most once."""
    pool = [(seq(rs, int(rs.choice(lengths))), seq(rs, int(rs.choice(lengths)))) for _ in range(n)]
    pick = np.minimum((rs.pareto(0.6, n) * 3).astype(np.int64), n - 1)      # index 0 .. : small indices come back often
    pick[rs.rand(n) < 0.6] = -1                                              # ... and most records are their own key
    m1, m2 = [], []
    for i in range(n):
        a, b = pool[i] if pick[i] < 0 else pool[int(pick[i]) % 64]
        m1.append((a, qual(rs, len(a))))
        m2.append((b, qual(rs, len(b))))
    return (fq(m1, b"s"), fq(m2, b"s")) if paired else (fq(m1, b"s"), None)


def own_inputs():
    f = {}
    for L in SE_LENGTHS:
        f["se_L%d" % L] = (single_shape(np.random.RandomState(1000 + L), L), None)
    for L1 in PE_LENGTHS:
        for L2 in PE_LENGTHS:
            f["pe_%d_%d" % (L1, L2)] = pair_shape(np.random.RandomState(100000 + 1000 * L1 + L2), L1, L2)
    rs = np.random.RandomState(7)
    # the concatenation seam: AC/GT and ACG/T are one key, A/CGT too; ACGT/"" cannot be written (L2 = 0)
    f["pe_seam"] = (fq([(b"AC", b"II"), (b"ACG", b"III"), (b"A", b"I"), (b"AC", b"II")]), fq([(b"GT", b"II"), (b"T", b"I"), (b"CGT", b"III"), (b"GA", b"II")]))
    # bytes: lower case is another key and the same matrix row; N and '.' share row 4; any other byte counts as T and is itself in the key
    odd = [b"ACGTNacgtn.", b"acgtnACGTN.", b"ACGTNacgtn.", b"ACGTNacgtn,", b"XYZ*-uU~!R0", b"xyz*-uU~!R0", b"ACGTNACGTN.", b"UUUUUUUUUUU", b"TTTTTTTTTTT"]
    f["se_bytes"] = (fq([(s, qual(rs, len(s))) for s in odd]), None)
    f["pe_bytes"] = (fq([(s, qual(rs, len(s))) for s in odd]), fq([(s, qual(rs, len(s))) for s in reversed(odd)]))
    reads = [seq(rs, 60) for _ in range(4)]
    reads = reads + reads[:2]
    f["se_crlf"] = (fq([(s, qual(rs, 60)) for s in reads], eol=b"\r\n"), None)      # the '\r' is the sequence's last byte: L = 61, a T
    f["pe_crlf"] = (fq([(s, qual(rs, 60)) for s in reads], eol=b"\r\n"), fq([(s[::-1], qual(rs, 60)) for s in reads], eol=b"\r\n"))
    # quality lines walked over their own length: shorter than the sequence, longer (up to 300), empty
    rag = [(seq(rs, 40), qual(rs, 40)), (seq(rs, 40), qual(rs, 7)), (seq(rs, 40), qual(rs, 300)), (seq(rs, 100), b""), (seq(rs, 300), qual(rs, 299)),
           (seq(rs, 1), qual(rs, 2)), (seq(rs, 150), qual(rs, 150))]
    f["se_ragged"] = (fq(rag), None)
    f["pe_ragged"] = (fq(rag), fq(list(reversed(rag))))
    f["pe_ragged_mate2"] = (fq([(s, qual(rs, len(s))) for s, _ in rag]), fq(rag))      # mate 1 regular, mate 2 not
    f["se_empty_quals"] = (fq([(seq(rs, 30), b"") for _ in range(5)]), None)
    # scale seams
    f["se_skew20k"] = skewed(np.random.RandomState(20), 20000, [60, 100, 150], False)
    f["pe_skew6k"] = skewed(np.random.RandomState(21), 6000, [40, 60, 76, 100], True)
    for n in (TILE - 1, TILE, TILE + 1):
        rs = np.random.RandomState(3000 + n)
        pool = [seq(rs, 20) for _ in range(300)]
        f["se_tile%d" % n] = (fq([(pool[int(k)], qual(rs, 20)) for k in rs.randint(0, 300, n)]), None)
    rs = np.random.RandomState(9)
    f["se_one"] = (fq([(b"ACGT", b"IIII")]), None)
    f["se_none"] = (b"", None)
    f["pe_none"] = (b"", b"")
    # no answer
    ok = [(seq(rs, 30), qual(rs, 30)) for _ in range(6)]
    put = lambda k, r: ok[:k] + [r] + ok[k + 1:]
    f["bad_len0"] = (fq(put(3, (b"", b""))), None)
    f["bad_len301"] = (fq(put(2, (seq(rs, 301), qual(rs, 301)))), None)
    f["bad_qual301"] = (fq(put(4, (seq(rs, 30), qual(rs, 301)))), None)
    f["bad_seq_byte"] = (fq(put(1, (b"ACGT\x80ACGT", qual(rs, 9)))), None)
    f["bad_qual_byte"] = (fq(put(5, (seq(rs, 9), b"IIII\x80IIII"))), None)
    f["bad_pe_mate2_len"] = (fq(ok), fq(put(2, (seq(rs, 301), qual(rs, 30)))))
    f["bad_pe_mate2_byte"] = (fq(ok), fq(put(0, (seq(rs, 30), b"\xff" + qual(rs, 29)))))
    f["bad_pe_both"] = (fq(put(4, (b"", b""))), fq(put(3, (seq(rs, 30), qual(rs, 301)))))      # mate 2's record 3 comes first
    f["bad_pe_short"] = (fq(ok), fq(ok[:5]))                                                     # mate 2 one record short
    f["pe_long"] = (fq(ok[:5]), fq(ok))                                                          # mate 2 one record long: ignored
    return f


def digest(data):
    return hashlib.sha256(data).hexdigest()


def digests(files=None):
    files = files or own_inputs()
    return {name + "." + str(m + 1): digest(t) for name, mates in files.items() for m, t in enumerate(mates) if t is not None}


def materialize(directory, expect=None):
    """Writes every input as NAME.1.fq (and NAME.2.fq) into `directory`; with `expect` ({"NAME.m": sha256}) checks each one first."""
    files = own_inputs()
    got = digests(files)
    if expect is not None:
        assert got == expect, sorted(k for k in set(got) | set(expect) if got.get(k) != expect.get(k))
    for name, mates in files.items():
        for m, t in enumerate(mates):
            if t is not None:
                with open(os.path.join(directory, "%s.%d.fq" % (name, m + 1)), "wb") as fh:
                    fh.write(t)
    return got
