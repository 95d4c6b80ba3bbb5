"""Python restatement of gzfastq_sort: framing (uniq_ref.records: the reference reads a record with the same four gzgets),
the order -- key line's length, then its bytes as unsigned, equal keys in input order -- the output format, stderr, and the
bookkeeping of the device's refinement sort (docs/kernels/fastq_sort.md): `rounds` and the records each round worked on.

Held to the recorded reference outputs by test_sort_golden.py; the GPU tests then use it as the checker for random inputs.
Where the reference has no answer (it crashes, or writes outside its array) `NoAnswer` is raised."""
from uniq_ref import NoAnswer, _Gz, records

FIRST_BYTES, WORD_BYTES, MAX_ROUNDS = 6, 8, 128


def count_read(data: bytes) -> int:
    """count_read: one per group of four gzgets whose first one returned a line."""
    gz, n = _Gz(data), 0
    while gz.gets() is not None:
        gz.gets(), gz.gets(), gz.gets()
        n += 1
    return n


def parse_r(arg: str) -> int:
    """str2unsigned_long: the leading digits ('-...' leaves with status 1 before anything is read)."""
    n = 0
    for ch in arg:
        if not "0" <= ch <= "9":
            break
        n = n * 10 + ord(ch) - 48
    return n % (1 << 64)


def order_of(keys):
    return sorted(range(len(keys)), key=lambda i: (len(keys[i]), keys[i]))   # (sorted is stable)


def refinement(keys, order=None):
    """[tied_0, tied_1, ...]: the records that are still undecided after round k (round k + 1 sorts those, the last entry's
    successor would be 0 and is left out).  Round 0 takes all records by (length, first 6 bytes); after round k
    a run -- the records that agree in length and in their first min(length, c_k) bytes, c_k = 6 + 8 k -- stays iff it has two
    or more records, its length exceeds c_k and its keys are not all equal.  Read off the final order, of which every run is
    a stretch (first key == last key there means all equal)."""
    n = len(keys)
    if not n:
        return []
    order = order_of(keys) if order is None else order
    tied, c, runs = [], FIRST_BYTES, [(0, n)]
    while True:
        nxt = []
        for a, b in runs:
            i = a
            while i < b:
                k = keys[order[i]]
                j = i + 1
                while j < b and len(keys[order[j]]) == len(k) and keys[order[j]][:c] == k[:c]:
                    j += 1
                if j - i >= 2 and len(k) > c and keys[order[j - 1]] != k:
                    nxt.append((i, j))
                i = j
        if not nxt:
            return tied
        tied.append(sum(b - a for a, b in nxt))
        runs, c = nxt, c + WORD_BYTES


class Result:
    pass


def simulate(data: bytes, by_name=False, r=None, rewindable=True, bookkeeping=True):
    """(output text, stderr with the times masked, Result) of `gzfastq_sort -i FILE [-n] [-r R]` on the inflated text `data`.
    r: the parsed -r (None or 0: absent).  rewindable: False for a pipe, which gzrewind cannot take back to its start."""
    res = Result()
    err = ""
    if not r:
        total = count_read(data)
        err += "total_reads_num: %d\nmax_reads_num: %d\n" % (total, total)
        if not rewindable:
            data = b""
    err += "name: %d\tseq: %d\n" % (int(by_name), int(not by_name))
    recs = list(records(data))
    if r and r < len(recs):
        raise NoAnswer("-r below the number of reads: the reference writes behind its array")
    keys = [x[0] if by_name else x[1] for x in recs]
    order = order_of(keys)
    out = b"".join(b"%s\n%s\n+\n%s\n" % recs[i] for i in order)
    err += "done read file at T s\ndone qsort file at T s\ndone write file at T s\n"
    res.n = len(recs)
    res.order = order
    if bookkeeping:
        res.tied = refinement(keys, order)
        res.rounds, res.refined = (1 + len(res.tied) if recs else 0), sum(res.tied)
        assert res.rounds <= MAX_ROUNDS
    return out, err, res
