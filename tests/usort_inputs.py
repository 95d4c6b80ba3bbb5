"""The inputs of tests/golden/usort/ that are not files of tests/golden/fastq/: made here, from fixed seeds, every time they are
needed -- by tests/golden/make_golden_usort.py when it records the reference, and by the tests, which write them into a temporary
directory and hold each one to the SHA-256 the recorder stored in the manifest.  Generators of gzfastq_uniq's and gzfastq_uniqQ's
goldens are used as they are; what gzfastq_uniq_sort needs beyond them is added here."""
import os

import numpy as np

import uniq_inputs
import uniqq_inputs
from uniq_inputs import ACGT, digest, fq, pool_of

KEY_LENGTHS = (0, 3, 4, 10, 11, 12, 15, 16, 17, 31, 32, 33, 300)   # 5381 * 33^L passes 2^32 at L = 4 and 2^64 at L = 11
TIE_US = (2047, 2048, 2049)


def qual(rs, n):
    return bytes(rs.randint(33, 74, n).astype(np.uint8))


def plain(n, seed=40):
    """n distinct reads of 12 bases: e = n."""
    rs = np.random.RandomState(seed + n)
    return fq([(b"@n%d" % i, s, qual(rs, 12)) for i, s in enumerate(pool_of(rs, n, 12, 12))])


def ties(u):
    """u keys of 2 .. 24 bases, key k in 2 + k % 2 shuffled copies: half of the keys share each count, so the order among them is
    slot, then first ordinal descending -- over a table of int(1.34 * 2.5 u) slots, in which chains of two and more are common."""
    rs = np.random.RandomState(700 + u)
    pool = pool_of(rs, u, 2, 24)
    idx = [k for k in range(u) for _ in range(2 + k % 2)]
    rs.shuffle(idx)
    return fq([(b"@p%d 1" % i, pool[k], qual(rs, len(pool[k]))) for i, k in enumerate(idx)])


def half(n=200):
    """One key carries n / 2 of the n records, the others one each."""
    rs = np.random.RandomState(41)
    pool = pool_of(rs, n // 2 + 1, 18, 22)
    idx = [0] * (n // 2) + list(range(1, n // 2 + 1))
    rs.shuffle(idx)
    return fq([(b"@h%d" % i, pool[k], qual(rs, len(pool[k]))) for i, k in enumerate(idx)])


def keylens():
    """Two keys of every length of KEY_LENGTHS, each twice (the empty key four times), shuffled behind a first record of 12
    bases: strLen = 12, and keys shorter and longer than it follow."""
    rs = np.random.RandomState(42)
    pool = [bytes(rs.choice(ACGT, L)) for L in KEY_LENGTHS for _ in range(2)]
    idx = list(range(len(pool))) * 2
    rs.shuffle(idx)
    recs = [(b"@k%d" % i, pool[k], qual(rs, len(pool[k]))) for i, k in enumerate(idx)]
    return fq([(b"@first", bytes(rs.choice(ACGT, 12)), qual(rs, 12))] + recs)


def empty_first():
    """The first two reads have no base: strLen is the length of the first read that has one."""
    rs = np.random.RandomState(43)
    seqs = [b"", b"", b"ACGTA", b"ACGTACGT", b"AC", b"", b"ACGTA", b"GGGTTTAAACCC", b"AC", b"T", b"ACGTACGT", b"GATTACA"]
    return fq([(b"@e%d" % i, s, qual(rs, len(s))) for i, s in enumerate(seqs)])


def pairs_mixed():
    """Pairs behind a first pair of 10 + 10 bases: mate 1 of 6 bases (the mate-1 line borrows four bytes of sequence 2), of 14
    (the mate-2 line starts with the tail of sequence 1) and of 10; every joined key has at least 10 bytes."""
    rs = np.random.RandomState(44)
    keys = [(bytes(rs.choice(ACGT, a)), bytes(rs.choice(ACGT, b))) for a, b in ((10, 10), (6, 9), (14, 3), (10, 0), (6, 4), (14, 20), (0, 10), (0, 25), (16, 16), (33, 31))]
    idx = [0] + [int(rs.randint(0, len(keys))) for _ in range(59)]
    r1 = [(b"@m%d 1" % i, keys[k][0], qual(rs, len(keys[k][0]))) for i, k in enumerate(idx)]
    r2 = [(b"@m%d 2" % i, keys[k][1], qual(rs, len(keys[k][1]))) for i, k in enumerate(idx)]
    return fq(r1), fq(r2)


def pairs_dups(n=3000, u=2400, seed=45):
    """n pairs of 20 + 20 bases over about u keys; the same bytes cut at another place are the same key."""
    rs = np.random.RandomState(seed)
    pool = pool_of(rs, u, 40, 40)
    r1, r2 = [], []
    for i in range(n):
        s = pool[int(rs.randint(0, u))]
        cut = 20 if i % 7 else 24
        r1.append((b"@d%d 1" % i, s[:cut], qual(rs, cut)))
        r2.append((b"@d%d 2" % i, s[cut:], qual(rs, 40 - cut)))
    return fq(r1), fq(r2)


def pairs30():
    rs = np.random.RandomState(46)
    pool = pool_of(rs, 8, 15, 15)
    r1, r2 = [], []
    for i in range(30):
        s, t = pool[int(rs.randint(0, 8))], pool[int(rs.randint(0, 3))]
        r1.append((b"@q%d 1" % i, s, qual(rs, 15)))
        r2.append((b"@q%d 2" % i, t, qual(rs, 15)))
    bad = [(b"@x15 2", s, q) if i == 15 else (n, s, q) for i, (n, s, q) in enumerate(r2)]
    return {"pe30_1.fq": fq(r1), "pe30_2.fq": fq(r2), "pe30_2bad15.fq": fq(bad), "pe30_2short.fq": fq(r2[:20]),
            "pe30_2long.fq": fq(r2 + [(b"@extra", b"ACGT", b"IIII")])}


def own_inputs():
    base = uniq_inputs.own_inputs()
    files = {name: base[name] for name in ("dups5000.fq", "hibytes.fq")}
    for n in (9, 10, 11):
        files["n%d.fq" % n] = plain(n)
    files["lone_only.fq"] = b"@one line without its newline"                       # e = 1, no record
    files["lone10.fq"] = plain(9, seed=50) + b"@tail without newline"              # e = 10, nine records
    files["lone_nl.fq"] = plain(12, seed=51) + b"@tail\n"                          # the reader runs into the end
    for u in TIE_US:
        files["ties_u%d.fq" % u] = ties(u)
    files["widths.fq"] = uniqq_inputs.widths()
    files["half.fq"] = half()
    files["keylens.fq"] = keylens()
    files["empty_first.fq"] = empty_first()
    files["crlf12.fq"] = fq([(b"@c%d" % i, [b"ACGT", b"GG", b"ACGTT"][i % 3], [b"IIII", b"55", b"IIII5"][i % 3]) for i in range(12)]).replace(b"\n", b"\r\n")
    files["nonl12.fq"] = fq([(b"@l%d" % i, [b"ACGT", b"GG"][i // 6], [b"IIII", b"55"][i // 6]) for i in range(12)])[:-1]
    files["shortq12.fq"] = fq([(b"@s%d" % i, b"ACGTAC"[:4 + i % 3], b"II"[:i % 3]) for i in range(12)])
    files["pm_1.fq"], files["pm_2.fq"] = pairs_mixed()
    files["pd_1.fq"], files["pd_2.fq"] = pairs_dups()
    files.update(pairs30())
    # undefined by construction: a pair's key shorter than strLen; a joined key of more than 1023 bytes
    rs = np.random.RandomState(47)
    a = [(b"@u%d 1" % i, b"ACGTACGTAC" if i != 7 else b"AC", b"IIIIIIIIII" if i != 7 else b"II") for i in range(12)]
    b = [(b"@u%d 2" % i, b"GGG", b"555") for i in range(12)]
    files["pshort_1.fq"], files["pshort_2.fq"] = fq(a), fq(b)
    s1, s2 = bytes(rs.choice(ACGT, 600)), bytes(rs.choice(ACGT, 424))
    files["plong_1.fq"] = fq([(b"@w%d 1" % i, s1 if i == 5 else s1[:30], b"I" * (600 if i == 5 else 30)) for i in range(12)])
    files["plong_2.fq"] = fq([(b"@w%d 2" % i, s2 if i == 5 else s2[:30], b"I" * (424 if i == 5 else 30)) for i in range(12)])
    files["p1023_1.fq"] = fq([(b"@w%d 1" % i, s1 if i == 5 else s1[:30], b"I" * (600 if i == 5 else 30)) for i in range(12)])
    files["p1023_2.fq"] = fq([(b"@w%d 2" % i, s2[:423] if i == 5 else s2[:30], b"I" * (423 if i == 5 else 30)) for i in range(12)])
    return files


def materialize(directory, digests=None):
    """Writes every input into `directory`; with `digests` ({name: sha256}) checks each one first."""
    files = own_inputs()
    if digests is not None:
        assert sorted(files) == sorted(digests), sorted(set(files) ^ set(digests))
    for name, data in files.items():
        if digests is not None:
            assert digest(name, data) == digests[name], name
        with open(os.path.join(directory, name), "wb") as f:
            f.write(data)
    return {name: digest(name, data) for name, data in files.items()}
