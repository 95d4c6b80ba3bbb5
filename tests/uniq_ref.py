"""Python restatement of gzfastq_uniq: framing, keys, representatives, the order of the hash-table walk (in closed
form) and the output format.

Held to the recorded reference outputs by test_uniq_golden.py; the GPU tests then use it as the checker for random
inputs.  Where the reference has no answer (it crashes, or reads outside its buffers) `NoAnswer` is raised.

The walk of dict.c in closed form.  The table starts with 4 buckets and doubles when it is full; a doubling walks the
old chains head to tail and pushes every entry onto its new chain's head, so it reverses them; new keys go to the head.
With h = djb2 of the key, j = the key's rank by first occurrence (0-based), e(j) = 0 for j < 4 else floor(log2 j) - 1,
U keys:  S = smallest power of two >= max(U, 4) (0 when U = 0), K = e(U - 1).  One exception: dictReplace tries dictAdd
first, and that doubles a full table before it finds the key -- so when U is a power of two >= 4 and a record BEHIND
the last first occurrence replaces its key's representative, S = 2 U and K = e(U - 1) + 1.  The keys come in ascending
(h & (S - 1), p, p ? j : -j) with p = (K - e(j)) & 1.
"""


class NoAnswer(ValueError):
    pass


class _Gz:
    """gzgets(file, buf, 1024) and gzeof over bytes."""

    def __init__(self, data: bytes):
        self.data, self.pos, self.past = data, 0, False

    def gets(self):
        d, a = self.data, self.pos
        if a >= len(d):
            self.past = True
            return None
        nl = d.find(b"\n", a, a + 1023)
        if nl >= 0:
            b = nl + 1
        else:
            b = min(a + 1023, len(d))
            if b == len(d) and b - a < 1023:
                self.past = True
        self.pos = b
        return d[a:b]


def _cstr(line):
    """What strlen sees of a line that gzgets returned."""
    if line is None:
        raise NoAnswer("the stream ends inside a record")
    if len(line) == 1023 and not line.endswith(b"\n"):
        raise NoAnswer("line of 1023 or more characters")
    z = line.find(b"\0")
    s = line if z < 0 else line[:z]
    if not s:
        raise NoAnswer("line that starts with a NUL byte")
    return s


def records(data: bytes):
    """readNextNode until it returns NULL: (name, sequence, quality) with the last byte of each line dropped."""
    gz = _Gz(data)
    while True:
        l1 = gz.gets()
        if gz.past:
            return
        name = _cstr(l1)[:-1]
        seq = _cstr(gz.gets())[:-1]
        if gz.gets() is None:
            raise NoAnswer("the stream ends inside a record")
        qual = _cstr(gz.gets())[:-1]
        yield name, seq, qual


def frame(data: bytes):
    return list(records(data))


def sum_q(seq: bytes, qual: bytes) -> int:
    if len(qual) + 1 < len(seq):
        raise NoAnswer("quality line two or more bytes shorter than the sequence")
    return sum(qual[:len(seq)])   # (one byte shorter: the terminating NUL adds 0)


def djb2(key: bytes) -> int:
    h = 5381
    for c in key:
        h = (h * 33 + c) & 0xFFFFFFFF
    return h


def epoch(j: int) -> int:
    return 0 if j < 4 else j.bit_length() - 2


class Result:
    pass


def collapse(data1: bytes, data2: bytes = None) -> Result:
    """The table after load_fastq_SE / _PE."""
    r = Result()
    r.paired = data2 is not None
    r.first, r.count, r.best, r.recs, r.error = {}, {}, {}, [], None
    it1 = records(data1)
    it2 = records(data2) if r.paired else None
    last_new = last_replace = -1
    for i, rec1 in enumerate(it1):
        if r.paired:
            rec2 = next(it2, None)
            n1 = rec1[0]
            sp = n1.find(b" ")
            bad = rec2 is None
            if not bad:
                bad = n1 != rec2[0] if sp < 0 else n1[:sp] != rec2[0][:sp]
            if bad:
                r.error = (i, n1)
                break
            key = rec1[1] + rec2[1]
            sq = (sum_q(rec1[1], rec1[2]) + sum_q(rec2[1], rec2[2])) & 0xFFFFFFFF
            r.recs.append((rec1, rec2))
        else:
            key = rec1[1]
            sq = sum_q(rec1[1], rec1[2]) & 0xFFFFFFFF
            r.recs.append((rec1,))
        if key not in r.first:
            r.first[key], r.count[key], r.best[key] = len(r.first), 1, (sq, i)
            last_new = i
        else:
            r.count[key] += 1
            if sq > r.best[key][0]:
                r.best[key] = (sq, i)
                last_replace = i
    r.n = len(r.recs)
    U = r.u = len(r.first)
    S, K = 0, 0
    if U:
        S = 4
        while S < U:
            S *= 2
        K = epoch(U - 1)
        if U >= 4 and U & (U - 1) == 0 and last_replace > last_new:
            S, K = 2 * S, K + 1
    r.hash_size, r.extra_doubling = S, bool(U >= 4 and U & (U - 1) == 0 and last_replace > last_new)

    def place(key):
        j = r.first[key]
        p = (K - epoch(j)) & 1
        return (djb2(key) & (S - 1), p, j if p else -j)

    r.table_order = sorted(r.first, key=place)
    r.key_order = sorted(r.first)
    return r


def render(r: Result, keys, mate=0) -> bytes:
    out = []
    for k in keys:
        name, seq, qual = r.recs[r.best[k][1]][mate]
        out.append(b"%s\t%d\n%s\n+\n%s\n" % (name, r.count[k], seq, qual))
    return b"".join(out)


def stderr_text(r: Result) -> str:
    err = ""
    if r.error:
        err += "error at %d: %s\nunmatched read name\n" % (r.error[0], r.error[1].decode("latin-1"))
    pct = "-nan" if r.n == 0 else "%.3f" % (100.0 * r.u / r.n)
    err += "unique reads number = %d(%d / %d = %s%%)\nhash size: %d\n" % (r.u, r.u, r.n, pct, r.hash_size)
    return err + "Finished load hash at T s\nFinished  at T s\n"


def simulate(data1: bytes, data2: bytes = None):
    """The whole tool: ({output suffix: bytes}, stderr as latin-1 text with the run times as 'T')."""
    r = collapse(data1, data2)
    if r.paired:
        out = {"_1_uniq.fq": render(r, r.table_order, 0), "_2_uniq.fq": render(r, r.table_order, 1)}
    else:
        out = {"_uniq.fq": render(r, r.table_order), "_sortKeyUniq.fq": render(r, r.key_order)}
    return out, stderr_text(r), r
