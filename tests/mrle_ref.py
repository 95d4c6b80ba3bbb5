"""Python restatement of gzfastq_mrle: framing (uniq_ref.records: the four gzgets of gzfastq_sort, input order), the two-pass
run-length codec over the six symbols  # / 7 < B F  (mrlec2), its decoder (mrled2, given the original length), the packed file
(one length byte modulo 256, then the encoded bytes), the decoded text, and what arrives on descriptor 1 when the packed file IS
standard output (a prefix that begins with '-'): two stdio streams with 4,096-byte buffers on one descriptor.

Held to the recorded reference outputs by test_mrle_golden.py; the GPU tests then use it as the checker for random inputs.  Where
the reference has no answer (it crashes, or a quality byte outside the six indexes an 8-entry table at 255) `NoAnswer` is raised."""
from uniq_ref import NoAnswer, records

SYMBOLS = b"#/7<BF"
INDEX = {c: i for i, c in enumerate(SYMBOLS)}
BUF = 4096
STDERR = "done read file at T s\nlist count: %d\ndone dump_array at T s\ndone sort file at T s\ndone write file at T s\ndone free list at T s\n"
PACKED, TEXT, SHARED = 0, 1, 2


def runs(line: bytes):
    """(symbol, length) of every maximal run."""
    out, a = [], 0
    for i in range(1, len(line) + 1):
        if i == len(line) or line[i] != line[a]:
            out.append((line[a], i - a))
            a = i
    return out


def savings(line: bytes):
    """t[0..5] behind pass 1: -1 for a run's first byte, +1 for every repeat whose count is no multiple of 255."""
    t = [0] * 6
    for c, n in runs(line):
        t[INDEX[c]] += n - 2 - (n - 1) // 255
    return t


def first_bad(quals):
    """The smallest ordinal of a quality line with a byte outside the six, or None."""
    for i, q in enumerate(quals):
        if q.strip(SYMBOLS):
            return i
    return None


def encode(line: bytes) -> bytes:
    if line.strip(SYMBOLS):
        raise NoAnswer("quality byte outside #/7<BF")
    t = savings(line)
    out = bytearray([sum((t[s] > 0) << s for s in range(6))])
    for c, n in runs(line):
        if t[INDEX[c]] > 0:
            k = (n - 1) // 255
            out += bytes([c]) + b"\xff" * k + bytes([n - 255 * k - 1])
        else:
            out += bytes([c]) * n
    return bytes(out)


def decode(enc: bytes, length: int) -> bytes:
    """mrled2: the flag byte, then symbols; behind a flagged one every 0xFF counts 255 and the first other byte v ends the run
    with v + 1."""
    flags, out, p = enc[0], bytearray(), 1
    while len(out) < length:
        c = enc[p]
        p += 1
        if (flags >> INDEX[c]) & 1:
            n = 0
            while enc[p] == 255:
                n += 255
                p += 1
            n += enc[p] + 1
            p += 1
            out += bytes([c]) * n
        else:
            out.append(c)
    assert p == len(enc)
    return bytes(out)


def shared(calls):
    """What descriptor 1 receives.  calls: (stream, bytes) in program order, stream 0 the text (stdout), 1 the packed file (a
    second FILE on the same descriptor).  A stream writes its next 4,096-byte block when a non-empty call does not fit into what
    is left of its buffer; fclose writes the packed stream's remainder, the text's remainder is lost (the process's exit flushes a
    stream whose descriptor fclose has closed)."""
    fed, flushed, whole, out = [0, 0], [0, 0], [bytearray(), bytearray()], bytearray()
    for s, b in calls:
        if not b:
            continue
        whole[s] += b
        fed[s] += len(b)
        while fed[s] - flushed[s] > BUF:
            out += whole[s][flushed[s]:flushed[s] + BUF]
            flushed[s] += BUF
    out += whole[1][flushed[1]:]
    return bytes(out)


def streams(quals):
    """(packed, text, shared) of the quality lines."""
    packed, text, calls = bytearray(), bytearray(), []
    for q in quals:
        e = encode(q)
        assert decode(e, len(q)) == q
        head = bytes([len(e) & 255])
        packed += head + e
        text += q + b"\n"
        calls += [(0, q), (0, b"\n"), (1, head), (1, e)]
    return bytes(packed), bytes(text), shared(calls)


def mrle(data: bytes, by_name=False):
    """((packed, text, shared), stderr with the times masked, number of records) of gzfastq_mrle on the inflated text."""
    quals = [r[2] for r in records(data)]
    bad = first_bad(quals)
    if bad is not None:
        raise NoAnswer("quality byte outside #/7<BF in record %d" % bad)
    err = "name: %d\tseq: %d\n" % (int(by_name), int(not by_name)) + STDERR % len(quals)
    return streams(quals), err, len(quals)
