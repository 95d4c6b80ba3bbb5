"""Python restatement of fastq2twobit and twoBit2seq: framing (uniq_ref.records: the reference reads a record with the same four
gzgets as gzfastq_sort), the reverse order of its list, the header, the codes, the zero padding; and the inverse: the header,
floor(body / packedLen) records from a zeroed buffer, seqlen characters and a newline each.

Held to the recorded reference outputs by test_twobit_golden.py; the GPU tests then use it as the checker for random inputs.
Where the reference has no answer (it crashes, indexes its table with a negative number, or never ends) `NoAnswer` is raised."""
import numpy as np

from uniq_ref import NoAnswer, records

CODE = bytearray(256)      # ntValNoN: T, U and every other byte 0
for _c, _v in ((b"cC", 1), (b"aA", 2), (b"gG", 3)):
    for _b in _c:
        CODE[_b] = _v
CODE = bytes(CODE)
NT = np.frombuffer(b"TCAG", np.uint8)      # valToNt
PACK_STDERR = "done read file at T s\nlist count: %d\ndone dump_array at T s\ndone sort file at T s\ndone write file at T s\ndone free list at T s\n"
UNPACK_STDERR = "done read file at T s\n"


def pack_seq(seq: bytes) -> bytes:
    """seq2sds: four bases per byte, the first in the top bits, the last byte's tail 0; nothing for an empty sequence."""
    if not seq:
        return b""
    c = np.frombuffer(seq.translate(CODE), np.uint8)
    c = np.concatenate([c, np.zeros(-len(c) % 4, np.uint8)]).reshape(-1, 4)
    return ((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8).tobytes()


def first_high(seqs):
    """The smallest ordinal of a sequence with a byte >= 0x80 (the reference's table index is a signed char), or None."""
    for i, s in enumerate(seqs):
        if s and max(s) >= 0x80:
            return i
    return None


def pack(data: bytes, by_name=False):
    """(output bytes, stderr with the times masked, number of records) of `fastq2twobit -i FILE [-n]` on the inflated text."""
    seqs = [r[1] for r in records(data)]
    bad = first_high(seqs)
    if bad is not None:
        raise NoAnswer("sequence byte of 0x80 or more in record %d" % bad)
    err = "name: %d\tseq: %d\n" % (int(by_name), int(not by_name)) + PACK_STDERR % len(seqs)
    if not seqs:
        return b"", err, 0
    last = seqs[-1]
    head = bytes([len(last) & 255, ((len(last) + 3) >> 2) & 255])
    return head + b"".join(pack_seq(s) for s in reversed(seqs)), err, len(seqs)


def unpack_records(seqlen: int, plen: int, body: bytes, n: int) -> bytes:
    """sds2seq over n records of plen bytes: record bytes behind plen read as 0."""
    if n == 0:
        return b""
    need = (seqlen + 3) >> 2
    rec = np.frombuffer(body, np.uint8, n * plen).reshape(n, plen)
    use = np.zeros((n, need), np.uint8)
    use[:, :min(need, plen)] = rec[:, :min(need, plen)]
    codes = np.stack([(use >> 6) & 3, (use >> 4) & 3, (use >> 2) & 3, use & 3], axis=2).reshape(n, need * 4)[:, :seqlen]
    text = np.full((n, seqlen + 1), 10, np.uint8)
    text[:, :seqlen] = NT[codes]
    return text.tobytes()


def unpack(blob: bytes):
    """(output text, stderr with the time masked) of `twoBit2seq -i FILE` on the file's bytes."""
    if len(blob) < 2:
        return b"", UNPACK_STDERR
    seqlen, plen = blob[0], blob[1]
    if plen == 0:
        raise NoAnswer("packedLen is 0: fread of 0 bytes never meets the end of the file")
    n = (len(blob) - 2) // plen      # a trailing partial record sets feof: dropped
    return unpack_records(seqlen, plen, blob[2:], n), UNPACK_STDERR
