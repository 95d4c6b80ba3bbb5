"""Inputs of map_kseq's recorded reference runs (tests/golden/make_golden_kseq.py) and of the tests that replay them: FASTA and
FASTQ text made from fixed seeds and fixed patterns, never stored -- the manifest holds their SHA-256.

The sequence lengths are the seams of the refinement sort (6 bytes in round 0, 8 more per round: c_k = 6 + 8 k) and one read
length; the record counts straddle the tiles of the kernels (kernels/kseq_frame.hip: 16 records or lines per workgroup where 16
lanes copy one, 64 per wave in the writer, 256 per workgroup elsewhere; kernels/radix_sort.hpp: 2048 items per scan tile).

FASTA as map_kseq reads it passes over every second header line (tests/kseq_ref.py), so the FASTA inputs that are about something
else put a filler block ">x\\nN\\n" behind every record: the filler is what is passed over."""
import gzip
import hashlib
import os
import random

LENGTHS = [1, 5, 6, 7, 8, 13, 14, 15, 22, 150]
TILES = [15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
HEADERS = [b"plain", b"blank ", b"tab\tcomment here", b"many   blanks  in it", b"cr\r", b" name of length zero", b"", b"two words", b"c \r", b"d x\r"]


def seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def fastq(recs, eol=b"\n", plus=b"+"):
    return b"".join(b"@" + h + eol + s + eol + plus + eol + q + eol for h, s, q in recs)


def wrap(s, width):
    return [s[i:i + width] for i in range(0, len(s), width)]


def fasta(recs, width=60, eol=b"\n", filler=True):
    out = []
    for h, s in recs:
        out.append(b">" + h + eol)
        out += [l + eol for l in wrap(s, width)]
        if filler:
            out.append(b">x" + eol + b"N" + eol)
    return b"".join(out)


def keyed(seed, one_length=None):
    """(header, sequence) pairs: every length of LENGTHS with a sequence, a proper prefix pair at that length, and duplicates
    under other names and comments, shuffled.  one_length: all sequences of that length instead (no prefix pairs)."""
    rng = random.Random(seed)
    seqs = []
    for n in ([one_length] * 12 if one_length else LENGTHS):
        s = seq(rng, n)
        seqs += [s, s]                                   # a duplicate
        if not one_length:
            seqs += [s + seq(rng, 1), s + seq(rng, 9)]   # s is a proper prefix of both
            if n > 1:
                seqs.append(s[:-1] + bytes([s[-1] ^ 0x20]))   # differs in its last byte only
    rng.shuffle(seqs)
    return [(b"r%d %s" % (i, b"c%d" % (i * 7 % 5)) if i % 3 else b"r%d" % i, s) for i, s in enumerate(seqs)]


def with_qual(pairs, seed):
    rng = random.Random(seed)
    return [(h, s, seq(rng, len(s), b"#5?IJ")) for h, s in pairs]


def counted(n, seed, length=8):
    """n records over about n / 2 distinct sequences of one length"""
    rng = random.Random(seed)
    pool = [seq(rng, length) for _ in range(max(1, n // 2))]
    return [(b"n%d" % i, rng.choice(pool)) for i in range(n)]


def own_inputs():
    """name -> bytes"""
    d = {}
    # ---- FASTQ shape
    d["fq_keys.fq"] = fastq(with_qual(keyed(1), 2))
    d["fq_one_length.fq"] = fastq(with_qual(keyed(3, one_length=22), 4))
    d["fq_high_bytes.fq"] = fastq(with_qual([(b"a", b"AC"), (b"b", b"\x80AC"), (b"c", b"\xffAC"), (b"d", b"AC\x80"), (b"e", b"ACG"), (b"f", b"AC\xff\xfe"),
                                             (b"g", b"\x7fAC"), (b"h", b"AC\x80"), (b"i", b"ACGTAC\x80ACGTACG\xff"), (b"j", b"ACGTAC\x80ACGTACGA")], 5))
    rng = random.Random(6)
    run = seq(rng, 22)
    d["fq_run_300.fq"] = fastq(with_qual([(b"o%d" % i, seq(rng, 22)) for i in range(10)] + [(b"run%d c%d" % (i, i), run) for i in range(300)] +
                                         [(b"p%d" % i, seq(rng, 22)) for i in range(10)], 7))
    d["fq_all_equal.fq"] = fastq(with_qual([(b"e%d" % i, b"ACGTACGTAC") for i in range(70)], 8))
    d["fq_all_distinct.fq"] = fastq(with_qual([(b"d%d" % i, b"%08d" % ((i * 7919) % 100000)) for i in range(300)], 9))
    d["fq_headers.fq"] = fastq(with_qual([(h, seq(rng, 9)) for h in HEADERS], 10))
    d["fq_crlf.fq"] = fastq(with_qual(keyed(11)[:20] + [(b"lone", b"\r")], 12), eol=b"\r\n")
    d["fq_qual_marker.fq"] = fastq([(b"a", b"ACGT", b"@III"), (b"b", b"CCGT", b">III"), (b"c", b"ACGT", b"+@@>"), (b"d", b"G", b"@")], plus=b"+name again")
    d["fq_nonl.fq"] = fastq(with_qual(keyed(13)[:9], 14))[:-1]
    for n in TILES:
        d["fq_n%d.fq" % n] = fastq(with_qual(counted(n, 100 + n), n))
    # one violation of each of the four conditions, and what else is not the shape
    ok = with_qual(keyed(15)[:6], 16)
    d["fq_v_line0.fq"] = fastq(ok[:3]) + b"Xr\nACGT\n+\nIIII\n" + fastq(ok[3:])
    d["fq_v_line1_empty.fq"] = fastq(ok[:3]) + b"@r\n\n+\n\n" + fastq(ok[3:])
    d["fq_v_line1_marker.fq"] = fastq(ok[:3]) + b"@r\n>CGT\n+\nIIII\n" + fastq(ok[3:])
    d["fq_v_line2.fq"] = fastq(ok[:3]) + b"@r\nACGT\nACGT\nIIII\n" + fastq(ok[3:])
    d["fq_v_line3.fq"] = fastq(ok[:3]) + b"@r\nACGT\n+\nIII\n" + fastq(ok[3:])
    d["fq_v_count.fq"] = fastq(ok) + b"\n"
    d["fq_wrapped.fq"] = b"".join(b"@" + h + b"\n" + s[:3] + b"\n" + s[3:] + b"\n+\n" + q[:2] + b"\n" + q[2:] + b"\n" for h, s, q in with_qual(keyed(17, one_length=8), 18))
    d["fq_truncated.fq"] = fastq(ok)[:-9]
    d["fq_minus2.fq"] = fastq(ok[:2]) + b"@r\nACGT\n+\nIIIIII\n" + fastq(ok[2:])
    # ---- FASTA shape
    for w in (1, 60, 70):
        d["fa_w%d.fa" % w] = fasta(keyed(20 + w) + [(b"long", seq(rng, 200))], w)
    d["fa_one_length.fa"] = fasta(keyed(24, one_length=150), 60)
    d["fa_nonl.fa"] = fasta(keyed(25)[:9], 7, filler=False)[:-1]
    d["fa_empty_lines.fa"] = b">a c\n\nACGT\n\n\nAC\n\n>x\n\nN\n\n>b\n\n\n>x\nN\n>c\nA\n\n"
    d["fa_empty_seq.fa"] = b">a\n>x\nN\n>b\nAC\n>x\nN\n>c d\n"
    d["fa_crlf.fa"] = fasta(keyed(26)[:15] + [(b"blank first", b"")], 5, eol=b"\r\n").replace(b">blank first\r\n", b">blank first\r\n\r\nACGT\r\n\r\nAC\r\n")
    d["fa_lone_cr.fa"] = b">whole\n\r\n>x\nN\n>first\n\r\nACGT\n>x\nN\n>second\nAC\n\r\nGT\n>x\nN\n>twice\n\n\r\n\r\nA\r\n>x\nN\n>crlf one\r\nA\r\n"
    d["fa_headers.fa"] = fasta([(h, seq(rng, 9)) for h in HEADERS], 60)
    d["fa_high_bytes.fa"] = fasta([(b"a", b"AC"), (b"b", b"\x80AC"), (b"c", b"\xffAC"), (b"d", b"AC\x80"), (b"e", b"ACG"), (b"f", b"ACGTAC\x80ACGTACG\xff")], 4)
    d["fa_passed_over.fa"] = fasta(keyed(27)[:11], 60, filler=False)
    d["fa_passed_over_hit.fa"] = fasta(keyed(27)[:3], 60, filler=False).replace(b">r1", b">r1 at@sign", 1) + b">z\nAC\n"
    d["fa_65535.fa"] = fasta([(b"big", seq(rng, 65535)), (b"small", b"ACGT")], 70)
    d["fa_65536.fa"] = fasta([(b"big", seq(rng, 65536)), (b"small", b"ACGT")], 70)
    for n in TILES:
        d["fa_n%d.fa" % n] = fasta(counted(n, 200 + n), 5)
    d["fa_cut_header.fa"] = fasta(keyed(28)[:3], 60) + b">cut"
    d["fa_cut_cr.fa"] = fasta(keyed(28)[:3], 60, filler=False) + b"\r"
    # ---- neither
    d["mixed.fx"] = b">a\nACGT\n@b\nACGT\n+\nIIII\n>c\nAC\n>d\nGG\n"
    d["text_in_front.fa"] = b"\n>a\nACGT\n"
    d["no_header.txt"] = b"no header in here\nnor here\n"
    d["nul.fq"] = b"@a\nAC\x00T\n+\nIIII\n"
    # ---- what the chunk tests cut at every byte
    d["cut_small.fa"] = b">a c\r\nACG\r\nT\r\n\r\n>x\r\nN\r\n>b\n\r\nAC\n>x y\nN\n>c\tz \nA\n\nC\n>x\nNN\n>d\nACG\r\n>x\nN\n>e\nACG"
    d["cut_small.fq"] = b"@a c\r\nACG\r\n+\r\nIII\r\n@b\n\r\n+b\n\r\n@c\tz \nAC\n+\n@>\n@\nACG\n+\n+II\n@e\nACG\n+\nIIJ"
    return d


def gz_inputs():
    """name -> the own input it is the one-member gzip of"""
    return {"fq_keys.fq.gz": "fq_keys.fq", "fa_w60.fa.gz": "fa_w60.fa", "fq_wrapped.fq.gz": "fq_wrapped.fq"}


def materialize(where):
    """Writes every own input (and the gzip members, mtime 0) into `where`; returns name -> SHA-256 of the plain inputs."""
    own = own_inputs()
    for name, text in own.items():
        with open(os.path.join(where, name), "wb") as f:
            f.write(text)
    for name, src in gz_inputs().items():
        with open(os.path.join(where, name), "wb") as f:
            f.write(gzip.compress(own[src], 6, mtime=0))
    return {name: hashlib.sha256(text).hexdigest() for name, text in own.items()}
