"""What map_kseq.cpp and kbtree_kseq.c do, restated in Python: klib's kseq_read over a record that is NEW for every call, the
two programs around it, and -- from the input alone -- the route the tools here must take (device or host).

kseq_read as the two programs call it (every call gets a zeroed kseq_t, only the stream is shared):
  * the call looks for the next '>' or '@' at ANY byte: the new record has forgotten that the sequence loop of the call before
    consumed the next header's first byte, so behind a FASTA record the next header line is passed over;
  * the name runs to the first isspace byte; unless that byte is '\\n' the rest of the line is the comment ('\\r' rule below),
    and a comment that the stream's end leaves without a byte to read stays NULL -> "(null)";
  * sequence lines are appended until a line starts with '>', '+' or '@' (that byte is consumed); empty lines are skipped;
  * the '\\r' rule: a line read to its end loses a trailing '\\r' when what has ACCUMULATED is longer than 1 byte; a line whose
    first byte is the stream's last byte is not read to its end and loses nothing;
  * no '+' line: FASTA, the quality is NULL -> "(null)"; else the rest of the '+' line is skipped (a stream that ends in it:
    -2) and quality lines are appended, at least one, until they reach the sequence's length; another length: -2;
  * both programs stop reading at the first negative return.
"""
SPACE = b" \t\n\v\f\r"
MAX = 65535


class Rec:
    __slots__ = ("name", "comment", "seq", "qual")


def _line(d, pos, acc):
    """the rest of the line at pos (at least one byte is there) appended to acc, its '\\n' passed, the '\\r' rule applied"""
    e = d.find(b"\n", pos)
    stop = len(d) if e < 0 else e
    acc += d[pos:stop]
    if len(acc) > 1 and acc.endswith(b"\r"):
        acc = acc[:-1]
    return acc, (len(d) if e < 0 else e + 1)


def kseq_records(d):
    """The records both programs read from the stream d, in order: Rec with comment / qual None where the pointer stays NULL."""
    out, pos, n = [], 0, len(d)
    while True:
        while pos < n and d[pos] not in b">@":
            pos += 1
        if pos == n:
            return out
        pos += 1
        if pos == n:
            return out
        i = pos
        while i < n and d[i] not in SPACE:
            i += 1
        r = Rec()
        r.name, r.comment, r.seq, r.qual = d[pos:i], None, b"", None
        stop = d[i] if i < n else 0
        pos = i + 1 if i < n else n
        if stop != 0x0A and pos < n:
            r.comment, pos = _line(d, pos, b"")
        plus = False
        while pos < n:
            c = d[pos]
            pos += 1
            if c in b">+@":
                plus = c == 0x2B
                break
            if c == 0x0A:
                continue
            r.seq += bytes([c])
            if pos < n:
                r.seq, pos = _line(d, pos, r.seq)
        if plus:
            e = d.find(b"\n", pos)
            if e < 0:
                return out   # -2
            pos = e + 1
            r.qual = b""
            while True:
                if pos == n:
                    break
                r.qual, pos = _line(d, pos, r.qual)
                if len(r.qual) >= len(r.seq):
                    break
            if len(r.qual) != len(r.seq):
                return out   # -2
        out.append(r)


def _text(first):
    return b"".join(r.name + b" " + (b"(null)" if r.comment is None else r.comment) + b"\n" + r.seq + b"\n+\n" +
                    (b"(null)" if r.qual is None else r.qual) + b"\n" for _, r in sorted(first.items()))


def map_kseq(d):
    """(stdout, stderr) of map_kseq on the stream d (a stream without NUL bytes)"""
    first = {}
    for r in kseq_records(d):
        first.setdefault(r.seq, r)   # std::map<std::string>: bytes as unsigned, a prefix first -- Python's order of bytes
    return _text(first), b"%d\n" % len(first)


def lengths(d):
    """the sequence lengths of the records read, in order of first appearance"""
    seen = []
    for r in kseq_records(d):
        if len(r.seq) not in seen:
            seen.append(len(r.seq))
    return seen


def kbtree_kseq(d):
    """(stdout, stderr) of kbtree_kseq where it has an answer -- every sequence of one length: map_kseq's; else None"""
    return map_kseq(d) if len(lengths(d)) <= 1 else None


# ---- the route -------------------------------------------------------------------------------------------------------------

def _rule(line):
    """a line's length after the '\\r' rule, standing alone"""
    return len(line) - (1 if len(line) > 1 and line.endswith(b"\r") else 0)


def _header_out(text):
    i = 0
    while i < len(text) and text[i] not in SPACE:
        i += 1
    if i == len(text):
        return i + 1 + 6
    c = text[i + 1:]
    return i + 1 + _rule(c)


def route(d):
    """"device" when the stream has one of the two shapes the device frames, else "host" -- from the input alone."""
    if not d:
        return "device"
    if 0 in d:
        return "host"   # (refused on either route)
    open_end = not d.endswith(b"\n")
    lines = d.split(b"\n")
    if not open_end:
        lines.pop()
    if d[0] == 0x40:   # FASTQ shape
        if len(lines) % 4:
            return "host"
        for k in range(0, len(lines), 4):
            h, s, p, q = lines[k:k + 4]
            if not h.startswith(b"@") or not s or s[0] in b">+@" or not p.startswith(b"+") or _rule(s) != _rule(q):
                return "host"
            if len(h) - 1 > MAX or len(s) > MAX or _header_out(h[1:]) > MAX:
                return "host"
        return "device"
    if d[0] != 0x3E:
        return "host"
    # FASTA shape: blocks open at the lines that start with '>'
    if any(l[:1] in (b"@", b"+") for l in lines):
        return "host"
    if open_end and (lines[-1].startswith(b">") or lines[-1] == b"\r"):
        return "host"
    blocks = []
    for l in lines:
        if l.startswith(b">"):
            blocks.append([l])
        else:
            blocks[-1].append(l)
    for b, blk in enumerate(blocks):
        if b & 1:   # passed over: no '>' or '@' behind its first byte
            body = b"\n".join(blk)[1:]
            if b">" in body or b"@" in body:
                return "host"
            continue
        acc = b""
        for l in blk[1:]:
            if l:
                acc += l
                if len(acc) > 1 and acc.endswith(b"\r"):
                    acc = acc[:-1]
        if len(blk[0]) - 1 > MAX or len(acc) > MAX or _header_out(blk[0][1:]) > MAX:
            return "host"
    return "device"


# ---- the ordering's bookkeeping ----------------------------------------------------------------------------------------------

def bookkeeping(d):
    """(rounds, refined) of the refinement sort in its bytes-only key mode over the records read from d: round 0 looks at the first
    6 bytes (zero-padded), every further round at 8 more; a run -- the records that agree in all bytes looked at -- is settled
    when its members are all equal, length included; `refined` sums the records of the unsettled runs over the rounds."""
    seqs = [r.seq for r in kseq_records(d)]
    if not seqs:
        return 0, 0

    def split(run, a, b):
        g = {}
        for s in run:
            g.setdefault(s[a:b].ljust(b - a, b"\0"), []).append(s)
        return [h for h in g.values() if len(set(h)) > 1]

    tied, c, rounds, refined = split(seqs, 0, 6), 6, 1, 0
    while tied:
        rounds, refined = rounds + 1, refined + sum(len(g) for g in tied)
        tied = [h for g in tied for h in split(g, c, c + 8)]
        c += 8
    return rounds, refined
