"""The inputs of tests/golden/uniqq/ that are not files of tests/golden/fastq/: made here, from fixed seeds, every time they
are needed -- by tests/golden/make_golden_uniqq.py when it records the reference, and by the tests, which write them into a
temporary directory and hold each one to the SHA-256 the recorder stored in the manifest.  The generators of gzfastq_uniq's
goldens (tests/uniq_inputs.py) are used as they are; what gzfastq_uniqQ needs beyond them is added here."""
import os

import numpy as np

import uniq_inputs
from uniq_inputs import digest, fq, pool_of

TIE_US = (3, 4, 5, 8, 9, 16, 17, 64, 65, 1025)


def parse(text):
    lines = text.split(b"\n")
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def equal_counts(u):
    """The with_u input of u keys cut down to the first record of every key, and those once more in reverse with other names
    and qualities: every count is 2, so -C's order is the table walk from its first group to its last."""
    seen, keep = set(), []
    for rec in parse(uniq_inputs.with_u(500 + u, u, False)[0]):
        if rec[1] not in seen:
            seen.add(rec[1])
            keep.append(rec)
    assert len(keep) == u
    return fq(keep + [(b"@again%d" % i, s, q[::-1]) for i, (n, s, q) in enumerate(reversed(keep))])


def ties(u):
    """u keys as with_u draws them, key k in 2 + k % 2 shuffled copies: half of the keys share each count, so -C's tie order is
    the table walk over many keys at every table size (with_u's own counts are random: at u = 3 no two are equal)."""
    rs = np.random.RandomState(600 + u)
    pool = pool_of(rs, u, 2, 24)
    idx = [k for k in range(u) for _ in range(2 + k % 2)]
    rs.shuffle(idx)
    return fq([(b"@p%d 1" % i, pool[k], bytes(rs.randint(34, 41, len(pool[k])).astype(np.uint8))) for i, k in enumerate(idx)])


def widths():
    """Counts 9, 10, 99 and 100 (and 1): the header's count takes one, two and three digits."""
    rs = np.random.RandomState(31)
    pool = pool_of(rs, 5, 6, 20)
    idx = [k for k, c in enumerate((9, 10, 99, 100, 1)) for _ in range(c)]
    rs.shuffle(idx)
    return fq([(b"@w%d" % i, pool[k], bytes(rs.randint(33, 74, len(pool[k])).astype(np.uint8))) for i, k in enumerate(idx)])


def ragged_group():
    """Groups whose members have names of 1 .. 300 bytes and quality lines of 0 .. 60 bytes, longer and shorter than the
    sequence (the quality sum is never printed, so a short line is regular)."""
    rs = np.random.RandomState(32)
    pool = pool_of(rs, 4, 0, 40)
    recs = []
    for i in range(64):
        s = pool[int(rs.randint(0, 4))]
        name = b"@" + bytes(rs.randint(48, 123, int(rs.choice([0, 1, 15, 16, 17, 40, 299]))).astype(np.uint8))
        recs.append((name, s, bytes(rs.randint(33, 127, int(rs.choice([0, 1, 15, 16, 17, 31, 32, 33, 60]))).astype(np.uint8))))
    return fq(recs)


def short_quals():
    return fq([(b"@a", b"ACGT", b"II"), (b"@b", b"ACGT", b"J"), (b"@c", b"ACGTAC", b""), (b"@d", b"ACGT", b"IIII"), (b"@e", b"ACGTAC", b"IIIIII")])


def own_inputs():
    base = uniq_inputs.own_inputs()
    files = {name: base[name] for name in ("dups5000.fq", "hibytes.fq", "crlf_dups.fq", "nonl_dups.fq", "lone_line.fq", "refine.fq")}
    for u in TIE_US:
        files["with_u%d.fq" % u] = uniq_inputs.with_u(500 + u, u, False)[0]
        files["ties_u%d.fq" % u] = ties(u)
    for u in (4, 5, 8, 9, 16, 17):
        files["equal_u%d.fq" % u] = equal_counts(u)
    files["widths.fq"] = widths()
    files["ragged_group.fq"] = ragged_group()
    files["short_quals.fq"] = short_quals()
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
