"""Inputs of the 2-bit pair's recorded reference runs (tests/golden/make_golden_twobit.py) and of the tests that replay them:
made from fixed seeds, never stored -- the manifest holds their SHA-256.  *.fq: FASTQ text for fastq2twobit; *.2bit: a header
and packed records for twoBit2seq."""
import hashlib
import os

import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
PACK_LENGTHS = list(range(10)) + [15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 1022]      # 256, 257, 1022: the header is modulo 256
UNPACK_SEQLENS = list(range(10)) + [63, 64, 65, 150, 255]
COUNTS = (0, 1, 2, 17)


def fq(recs):
    return b"".join(b"%s\n%s\n+\n%s\n" % r for r in recs)


def reads(seed, lengths, alphabet=ACGT):
    rs = np.random.RandomState(seed)
    return [(b"@r%d" % i, bytes(rs.choice(alphabet, n)), bytes(rs.randint(33, 74, n).astype(np.uint8))) for i, n in enumerate(lengths)]


def with_high_byte(recs, which):
    out = list(recs)
    for k in which:
        name, seq, qual = out[k]
        out[k] = (name, seq[:3] + b"\xe3" + seq[4:], qual)
    return out


def twobit(seqlen, plen, n, seed, tail=b""):
    """A header and n records of plen random bytes (every code in every position), `tail` behind them."""
    rs = np.random.RandomState(seed)
    return bytes([seqlen, plen]) + bytes(rs.randint(0, 256, n * plen).astype(np.uint8)) + tail


def own_inputs():
    f = {}
    for n in PACK_LENGTHS:
        f["len%d.fq" % n] = fq(reads(100 + n, [n]))
    f["all_lengths.fq"] = fq(reads(7, PACK_LENGTHS))
    f["mixed.fq"] = fq(reads(8, [150, 0, 3, 151, 16, 1, 149, 37, 4, 0]))                  # the last record empty: header 00 00
    f["mixed_last150.fq"] = fq(reads(9, [0, 7, 150, 2, 33, 150]))
    f["letters.fq"] = fq(reads(10, [40, 41, 42, 43, 5], np.frombuffer(b"ACGTacgtNnUuRYKM.-*", np.uint8)))
    f["crlf.fq"] = fq(reads(11, [12, 7, 8])).replace(b"\n", b"\r\n")                      # "ACGT\r" is a 5-byte sequence
    f["nonl.fq"] = fq(reads(12, [30, 31, 32]))[:-1]
    f["example.fq"] = fq([(b"@r1", b"ACGTA", b"IIIII"), (b"@r2", b"NNGGCCTTA", b"IIIIIIIII"), (b"@r3", b"acgtACGTX", b"IIIIIIIII")])
    plain = reads(13, [20] * 12)
    f["plain12.fq"] = fq(plain)
    f["hi_last.fq"] = fq(with_high_byte(plain, [11]))
    f["hi_first.fq"] = fq(with_high_byte(plain, [0]))
    f["hi_mid.fq"] = fq(with_high_byte(plain, [9, 5, 7]))
    for s in UNPACK_SEQLENS:
        f["u%d.2bit" % s] = twobit(s, (s + 3) >> 2, 3, 200 + s)                            # (u0: packedLen 0 -- the reference never ends)
    f["u0_p1.2bit"] = twobit(0, 1, 5, 230)
    for s, p in ((150, 1), (150, 20), (9, 1), (9, 2), (255, 63), (1, 1), (255, 1)):
        f["small_%d_%d.2bit" % (s, p)] = twobit(s, p, 4, 240 + s + p)
    for s, p in ((5, 3), (150, 40), (5, 255), (1, 255), (255, 255), (64, 17)):
        f["large_%d_%d.2bit" % (s, p)] = twobit(s, p, 4, 260 + s + p)
    for n in COUNTS:
        f["n%d.2bit" % n] = twobit(150, 38, n, 280 + n)
    f["partial.2bit"] = twobit(150, 38, 5, 290, tail=b"\x1b" * 37)
    f["partial_only.2bit"] = twobit(150, 38, 0, 291, tail=b"\x1b" * 20)
    f["bytes0.2bit"] = b""
    f["bytes1.2bit"] = b"\x05"
    f["bytes2.2bit"] = b"\x05\x02"
    f["zero_zero.2bit"] = b"\x00\x00"
    f["p0_data.2bit"] = b"\x05\x00" + b"\x1b\x1b\xe4\x00"
    f["issue_a.2bit"] = b"\x05\x01" + b"\x1b\x1b\xe4\x00"
    f["issue_b.2bit"] = b"\x03\x02" + b"\x1b\x1b\xe4"
    return f


def digest(data):
    return hashlib.sha256(data).hexdigest()


def materialize(directory, digests=None):
    """Writes every input into `directory`; with `digests` ({name: sha256}) checks each one first."""
    files = own_inputs()
    if digests is not None:
        assert sorted(files) == sorted(digests), sorted(set(files) ^ set(digests))
    for name, data in files.items():
        if digests is not None:
            assert digest(data) == digests[name], name
        with open(os.path.join(directory, name), "wb") as fh:
            fh.write(data)
    return {name: digest(data) for name, data in files.items()}
