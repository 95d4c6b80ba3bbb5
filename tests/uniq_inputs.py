"""The inputs of tests/golden/uniq/ that are not files of tests/golden/fastq/: made here, from fixed seeds, every time they
are needed -- by tests/golden/make_golden_uniq.py when it records the reference, and by the tests, which write them into a
temporary directory and hold each one to the SHA-256 the recorder stored in the manifest.  (Stored as files they were
56,000 lines of random reads.)"""
import gzip
import hashlib
import os

import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)


def fq(recs):
    return b"".join(n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def pool_of(rs, u, lo, hi, alphabet=ACGT):
    pool, seen = [], set()
    while len(pool) < u:
        s = bytes(rs.choice(alphabet, int(rs.randint(lo, hi + 1))))
        if s not in seen:
            seen.add(s)
            pool.append(s)
    return pool


def with_u(seed, u, replace_behind, pairs=False):
    """Exactly u keys; every key comes at least twice.  replace_behind: behind the last first occurrence some record
    beats its key's earlier quality sums (dict.c then doubles a full table once more); otherwise none does."""
    rs = np.random.RandomState(seed)
    pool = pool_of(rs, u, 2, 24)
    idx = list(range(u)) + [int(rs.randint(0, u)) for _ in range(u)]
    rs.shuffle(idx)
    seen, last_new = set(), 0
    for i, k in enumerate(idx):
        if k not in seen:
            seen.add(k)
            last_new = i
    tail = [int(rs.randint(0, u)) for _ in range(3)]
    idx += tail
    r1, r2 = [], []
    for i, k in enumerate(idx):
        s = pool[k]
        behind = i > last_new
        # in front of the last new key: qualities 33 .. 40 at random; behind it: the least (never a replacement) or, for
        # the very last record, the greatest possible
        if not behind:
            q = bytes(rs.randint(34, 41, len(s)).astype(np.uint8))
        elif replace_behind and i == len(idx) - 1:
            q = b"~" * len(s)
        else:
            q = b"!" * len(s)
        cut = int(rs.randint(0, len(s) + 1)) if pairs else len(s)
        r1.append((b"@p%d 1" % i, s[:cut], q[:cut]))
        r2.append((b"@p%d 2" % i, s[cut:], q[cut:]))
    return (fq(r1), fq(r2)) if pairs else (fq(r1), None)


def dups5000():
    rs = np.random.RandomState(3)
    pool = [bytes(rs.choice(np.frombuffer(b"ACGTN", np.uint8), int(rs.randint(0, 41)))) for _ in range(700)]
    recs = []
    for i in range(5000):
        s = pool[int(rs.randint(0, len(pool)))]
        recs.append((b"@r%d x:%d" % (i, i % 7), s, bytes(rs.randint(33, 74, len(s)).astype(np.uint8))))
    return fq(recs)


def refine():
    """Keys that differ only behind byte 8, 16 and 24, and keys that are prefixes of one another."""
    base = b"ACGTACGTTTGACCAGGGTACCATAGGCATTACG"
    seqs = [base[:k] for k in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 34)]
    for at in (8, 9, 16, 17, 24, 25, 33):
        for c in b"ACGT":
            seqs.append(base[:at] + bytes([c]) + base[at + 1:])
    rs = np.random.RandomState(5)
    order = list(range(len(seqs))) * 2
    rs.shuffle(order)
    return fq([(b"@f%d" % i, seqs[k], bytes(rs.randint(40, 70, len(seqs[k])).astype(np.uint8))) for i, k in enumerate(order)])


def equal_sums():
    recs = []
    for i in range(24):
        s = [b"ACGT", b"GGGTT", b"A"][i % 3]
        recs.append((b"@e%d" % i, s, (b"5I5I5"[:len(s)] if i % 2 else b"I5I55"[:len(s)])))   # the same sum in another order
    return fq(recs)


def hibytes():
    rs = np.random.RandomState(8)
    words = ["Probe-échantillon", "测序", "röd", "µL"]
    alphabet = np.frombuffer(bytes([65, 67, 71, 84, 0x80, 0xC3, 0xFF]), np.uint8)
    pool = pool_of(rs, 9, 1, 30, alphabet)
    recs = []
    for i in range(40):
        s = pool[int(rs.randint(0, 9))]
        recs.append((("@%s:%d %s" % (words[i % 4], i, words[(i + 1) % 4])).encode("utf-8"), s, bytes(rs.randint(33, 256, len(s)).astype(np.uint8)).replace(b"\n", b"!")))
    return fq(recs)


def pair_inputs():
    rs = np.random.RandomState(21)
    pool = pool_of(rs, 12, 4, 30)
    a, b, same = [], [], []
    for i in range(60):
        s, t = pool[int(rs.randint(0, 12))], pool[int(rs.randint(0, 4))]
        qa, qb = bytes(rs.randint(33, 74, len(s)).astype(np.uint8)), bytes(rs.randint(33, 74, len(t)).astype(np.uint8))
        a.append((b"@M01:77:%d 1:N:0" % i, s, qa))
        b.append((b"@M01:77:%d 2:N:0" % i, t, qb))
        same.append((b"@M01:77:%d 2:N:0" % i, s, qa))
    amb1 = [(b"@c%d 1" % i, [b"AC", b"A", b"", b"ACG"][i % 4], [b"II", b"5", b"", b"AAA"][i % 4]) for i in range(16)]
    amb2 = [(b"@c%d 2" % i, [b"G", b"CG", b"ACG", b""][i % 4], [b"I", b"I5", b"III", b""][i % 4]) for i in range(16)]
    bad_mid = [(b"@X01:77:%d 2:N:0" % i if i == 31 else n, s, q) for i, (n, s, q) in enumerate(b)]
    nospace_a = [(b"@n%d" % i, s, q) for i, (n, s, q) in enumerate(a[:20])]
    nospace_eq = [(b"@n%d" % i, s, q) for i, (n, s, q) in enumerate(b[:20])]
    nospace_ne = [(b"@n%d/2" % i if i == 11 else b"@n%d" % i, s, q) for i, (n, s, q) in enumerate(b[:20])]
    return {
        "pe_a.fq": fq(a), "pe_b.fq": fq(b), "pe_same.fq": fq(same), "pe_amb_1.fq": fq(amb1), "pe_amb_2.fq": fq(amb2),
        "pe_b_badmid.fq": fq(bad_mid), "pe_b_short.fq": fq(b[:37]), "pe_b_long.fq": fq(b + [(b"@extra%d" % i, b"ACGT", b"IIII") for i in range(5)]),
        "pe_ns_a.fq": fq(nospace_a), "pe_ns_eq.fq": fq(nospace_eq), "pe_ns_ne.fq": fq(nospace_ne), "pe_b.fq.gz": gzip.compress(fq(b), 6, mtime=0),
    }


def own_inputs():
    files = {"dups5000.fq": dups5000(), "refine.fq": refine(), "equal_sums.fq": equal_sums(), "hibytes.fq": hibytes()}
    files["crlf_dups.fq"] = fq([(b"@c%d" % i, [b"ACGT", b"GG"][i % 2], [b"IIII", b"55"][i % 2]) for i in range(6)]).replace(b"\n", b"\r\n")
    files["nonl_dups.fq"] = fq([(b"@l%d" % i, [b"ACGT", b"GG"][i // 3], [b"IIII", b"55"][i // 3]) for i in range(6)])[:-1]
    files["lone_line.fq"] = fq([(b"@l%d" % i, b"ACGT", b"IIII") for i in range(3)]) + b"@tail without newline"
    files["shortq.fq"] = fq([(b"@a", b"ACGT", b"IIII"), (b"@b", b"ACGTAC", b"IIII"), (b"@c", b"ACGT", b"IIII")])
    # NUL bytes: gzgets copies them, strlen stops at them, and the byte in front of the NUL is the one that is dropped
    files["nul_bytes.fq"] = (b"@a x\0junk\nACGT\0TT\n+\nIIII\0II\n@b\nACG\n+\nIII\n@c\nAC\0\n+\nI5\n@d y\nA\n+\n5\0\n" +
                             fq([(b"@e%d" % i, b"ACG", b"5I5") for i in range(3)]))
    files["fields3.fq"] = fq([(b"@SRR1.%d %d length=%d" % (i, i, 4 + i % 2), [b"ACGT", b"GGTCA"][i % 2], [b"IIII", b"55555"][i % 2]) for i in range(10)])
    for u in (3, 5, 9, 17, 33, 65, 129, 1025):
        files["u%d.fq" % u] = with_u(100 + u, u, False)[0]
    for u in (4, 8, 16, 32, 64, 128, 1024):
        files["u%d_plain.fq" % u] = with_u(200 + u, u, False)[0]
        files["u%d_behind.fq" % u] = with_u(300 + u, u, True)[0]
    for u in (4, 8, 16, 64):
        for kind in ("plain", "behind"):
            one, two = with_u(400 + u + (kind == "behind"), u, kind == "behind", pairs=True)
            files["pu%d_%s_1.fq" % (u, kind)], files["pu%d_%s_2.fq" % (u, kind)] = one, two
    files.update(pair_inputs())
    return files


def digest(name, data):
    """What the manifest holds of an input: the SHA-256 of its text (of a gzip file: of what it inflates to -- the
    compressed bytes may differ between zlib builds)."""
    return hashlib.sha256(gzip.decompress(data) if name.endswith(".gz") else data).hexdigest()


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
