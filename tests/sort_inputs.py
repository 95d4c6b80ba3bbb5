"""The inputs of tests/golden/sort/ that are not files of tests/golden/fastq/: made here, from fixed seeds, every time they
are needed -- by tests/golden/make_golden_sort.py when it records the reference, and by the tests, which write them into a
temporary directory and hold each one to the SHA-256 the recorder stored in the manifest."""
import gzip
import os

import numpy as np

from uniq_inputs import ACGT, digest, fq, pool_of

# key-line lengths on both sides of the refinement's word borders (6, 14, 22 bytes) and of gzgets' 1023-byte buffer
EDGE_LENGTHS = (5, 6, 7, 13, 14, 15, 21, 22, 23, 1021, 1022)


def quals(rs, n):
    return bytes(rs.randint(33, 74, n).astype(np.uint8))


def ties40(n=3000):
    """n reads drawn from 40 sequences of 5 to 12 bytes: many ties by sequence, every name and quality different."""
    rs = np.random.RandomState(40)
    pool = pool_of(rs, 40, 5, 12)
    recs = []
    for i in range(n):
        s = pool[int(rs.randint(0, 40))]
        recs.append((b"@t%d/%d" % (int(rs.randint(0, 10 ** int(rs.randint(1, 7)))), i), s, quals(rs, len(s))))
    return fq(recs)


def dup_names():
    """Few names, each many times, over different sequences and qualities: ties by name."""
    rs = np.random.RandomState(41)
    names = [b"@dup", b"@dup 1", b"@dup 2", b"@DUP", b"@d", b"@dup:long:name:with:fields 1:N:0", b"@dup:long:name:with:fields 2:N:0"]
    recs = []
    for i in range(400):
        ln = int(rs.randint(1, 40))
        recs.append((names[int(rs.randint(0, len(names)))], bytes(rs.choice(ACGT, ln)), quals(rs, ln)))
    return fq(recs)


def edges():
    """Names and sequences of the EDGE_LENGTHS, which agree up to their last byte, their last word, or not at all."""
    rs = np.random.RandomState(42)
    base = bytes(rs.choice(ACGT, 1022))
    recs = []
    for rep in range(3):
        for ln in EDGE_LENGTHS:
            for kind in range(4):
                s = bytearray(base[:ln])
                if kind == 1:
                    s[-1] = b"ACGT"[int(rs.randint(0, 4))]
                elif kind == 2:
                    s[max(ln - 9, 0)] = b"ACGT"[int(rs.randint(0, 4))]
                elif kind == 3:
                    s = bytearray(rs.choice(ACGT, ln))
                name = b"@" + bytes(s[:ln - 1]).lower()
                recs.append((name, bytes(s), quals(rs, ln if kind else max(ln - 3, 1))))
    order = rs.permutation(len(recs))
    return fq([recs[k] for k in order])


def illumina(n=2500):
    """Names with the long common prefix of one flow cell and lane, numbers of different widths, some names twice."""
    rs = np.random.RandomState(43)
    recs = []
    for i in range(n):
        tile = 1101 + int(rs.randint(0, 3))
        name = b"@A00123:456:HXXXXXXXX:1:%d:%d:%d %d:N:0:ACGTACGT" % (tile, int(rs.randint(1000, 1100)), int(rs.randint(900, 1100)), 1 + i % 2)
        ln = int(rs.choice([36, 50, 50, 50, 75]))
        recs.append((name, bytes(rs.choice(ACGT, ln)), quals(rs, ln)))
    return fq(recs)


def hibytes():
    rs = np.random.RandomState(44)
    words = ["Probe-échantillon", "测序", "röd", "µL", "\x7f\x80"]
    alphabet = np.frombuffer(bytes([1, 65, 67, 0x7F, 0x80, 0xC3, 0xFF]), np.uint8)
    pool = pool_of(rs, 30, 1, 30, alphabet)
    recs = []
    for i in range(200):
        s = pool[int(rs.randint(0, 30))]
        q = bytes(rs.randint(33, 256, len(s)).astype(np.uint8)).replace(b"\n", b"!")
        recs.append((("@%s:%d %s" % (words[i % 5], i % 17, words[(i + 1) % 5])).encode("latin-1", "replace") if i % 3 else ("@%s" % words[i % 5]).encode("utf-8"), s, q))
    return fq(recs)


def small():
    rs = np.random.RandomState(45)
    recs = []
    for i in range(12):
        ln = int(rs.randint(3, 9))
        recs.append((b"@s%d" % (i * 7 % 12), bytes(rs.choice(ACGT, ln)), quals(rs, ln)))
    return recs


def own_inputs():
    files = {"ties40.fq": ties40(), "dup_names.fq": dup_names(), "edges.fq": edges(), "illumina.fq": illumina(), "hibytes.fq": hibytes()}
    s = fq(small())
    files["small.fq"] = s
    files["small.fq.gz"] = gzip.compress(s, 6, mtime=0)
    files["ties40.fq.gz"] = gzip.compress(files["ties40.fq"], 6, mtime=0)
    files["crlf.fq"] = s.replace(b"\n", b"\r\n")
    files["nonl.fq"] = s[:-1]
    files["lone_line.fq"] = s + b"@tail without newline"
    files["shortq.fq"] = fq([(b"@a", b"ACGT", b"IIII"), (b"@b", b"ACGTAC", b"II"), (b"@c", b"ACGT", b"")])
    files["cut_plus.fq"] = s + b"@x\nACGT\n+\n"          # ends behind the '+' line
    files["cut_seq.fq"] = s + b"@x\nACGT\n"
    files["cut_name.fq"] = s + b"@x\n"
    files["one.fq"] = fq([(b"@only", b"ACGT", b"IIII")])
    files["nul_bytes.fq"] = b"@a x\0junk\nACGT\0TT\n+\nIIII\0II\n@b\nACG\n+\nIII\n@a x\nAC\0\n+\nI5\n" + s
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
