"""Inputs of gzfastq_mrle's recorded reference runs (tests/golden/make_golden_mrle.py) and of the tests that replay them: FASTQ
text whose quality lines use the six symbols  # / 7 < B F  (the codec's domain), made from fixed seeds and fixed patterns, never
stored -- the manifest holds their SHA-256."""
import hashlib
import os

import numpy as np

SYM = b"#/7<BF"
LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 1022]
RUNS = [1, 2, 254, 255, 256, 510, 511, 1022]


def fq(quals, seq=b"ACGT"):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, seq, q) for i, q in enumerate(quals))


def line(rs, n, mean_run=6):
    """n bytes over the six symbols in runs of geometric length (mean_run 1: hardly any run)."""
    out = bytearray()
    while len(out) < n:
        out += bytes([SYM[rs.randint(6)]]) * int(rs.geometric(1.0 / mean_run))
    return bytes(out[:n])


def lines(seed, lengths, mean_run=6):
    rs = np.random.RandomState(seed)
    return [line(rs, int(n), mean_run) for n in lengths]


def fill_text(total, seed):
    """Quality lines whose text stream (every line and its newline) has exactly `total` bytes."""
    rs, out, left = np.random.RandomState(seed), [], total
    while left:
        n = min(int(rs.randint(0, 200)), left - 1)
        out.append(line(rs, n))
        left -= n + 1
    return out


def savings_lines():
    """For every symbol s: savings of -1 (one single occurrence), 0 (one run of two; a run of three and a single one) and +1 (one
    run of three), s's runs apart from each other between single bytes of its neighbour."""
    out = []
    for i in range(6):
        s, o = SYM[i:i + 1], SYM[(i + 1) % 6:(i + 1) % 6 + 1]
        out += [o + s + o, o + s * 2 + o, s * 3 + o + s, o + s * 3 + o, s * 256 + o + s * 2]
    return out


def own_inputs():
    from mrle_ref import encode
    f = {}
    for n in LENGTHS:
        f["len%d.fq" % n] = fq(lines(100 + n, [n]))
    f["all_lengths.fq"] = fq(lines(7, LENGTHS))
    for n in RUNS:
        f["run%d.fq" % n] = fq([b"F" * n])
    f["all_runs.fq"] = fq([SYM[k % 6:k % 6 + 1] * n for k, n in enumerate(RUNS)])
    # runs across a lane's 16 bytes (positions 16, 32, ...) and a team's 256, alone and inside a longer run
    f["straddle.fq"] = fq([b"#" * 14 + b"F" * 4 + b"#" * 10, b"#" * 15 + b"F" * 2, b"F" * 16 + b"B" * 16 + b"F", b"<" * 250 + b"7" * 12 + b"/" * 300,
                           b"B" * 255 + b"F" * 2 + b"B", b"#/" * 127 + b"FFFF" + b"7<" * 100, b"F" * 240 + b"#" * 32 + b"F" * 500 + b"B" * 250])
    f["savings.fq"] = fq(savings_lines())
    f["flags_all.fq"] = fq([b"###///777<<<BBBFFF", b"F" * 300 + b"B" * 3 + b"<" * 3 + b"7" * 3 + b"/" * 3 + b"#" * 600])
    f["flags_none.fq"] = fq([b"#/7<BF" * 20, b"FF##BB", b""])
    sized = [b"F#" * 127, b"F#" * 127 + b"/", b"F#" * 128, b"F#" * 300, b"F" * 254 + b"#" + b"B" * 700]
    assert [len(encode(q)) for q in sized[:4]] == [255, 256, 257, 601]
    f["sizes.fq"] = fq(sized)
    f["mixed.fq"] = fq(lines(8, list(range(40)) + [150, 0, 3, 151, 16, 1, 149, 37, 4, 0]))      # packed and text offsets of every alignment
    f["mixed_noruns.fq"] = fq(lines(9, [150] * 30 + list(range(33)), mean_run=1))
    f["reads150.fq"] = fq(lines(10, [150] * 500, mean_run=12))
    f["one_empty.fq"] = fq([b""])
    f["last_empty.fq"] = fq([b"FFFF", b"##", b""])
    f["nonl.fq"] = fq(lines(12, [30, 31, 32]))[:-1]                                                # the last quality line loses its last byte
    f["examples.fq"] = fq([b"FFFFFFFF", b"FF##FF", b"FFF/77<<<BBBB", b"F" * 255, b"F" * 256, b"F" * 511, b"#" * 600])
    plain = lines(13, [20] * 12)
    f["plain12.fq"] = fq(plain)
    bad = lambda which: fq([q[:7] + b"I" + q[8:] if k in which else q for k, q in enumerate(plain)])
    f["bad_first.fq"], f["bad_mid.fq"], f["bad_last.fq"] = bad([0]), bad([9, 5, 7]), bad([11])
    # the shared descriptor: text streams of 4,095 / 4,096 / 4,097 / 8,192 bytes
    for total in (4095, 4096, 4097, 8192):
        f["text%d.fq" % total] = fq(fill_text(total, 300 + total))
    # a text call that ends exactly on a block edge (the line's last byte is byte 4,095, its newline opens the next block), more behind it
    f["edge_text.fq"] = fq([b"F#" * 511] * 4 + [b"FF##"] + lines(14, [100] * 60))
    # a packed call that ends exactly on a block edge: 16 records of 1 + 255 bytes, more behind them
    f["edge_packed.fq"] = fq([b"F#" * 127] * 16 + lines(15, [100] * 90))
    f["packed4096.fq"] = fq([b"F#" * 127] * 16)                                                    # the packed stream is one full buffer
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
