"""Python restatement of gzfastq_uniqQ: framing (uniq_ref.records -- the same readNextNode), the per-key lists, the two
orders and the output format.

Held to the recorded reference outputs by test_uniqq_golden.py; the GPU tests then use it as the checker for random
inputs.  Where the reference has no answer (it crashes) `NoAnswer` is raised -- and for a NUL byte in a line, which the
tool refuses as well.

Every record is put at the head of its key's list, so a key's members come out in reverse input order, and the group's
name is the last member's.  The tool only ever calls dictAdd, so the table has S = smallest power of two >= max(U, 4)
slots (0 without a record) and uniq_ref's extra doubling cannot happen; the walk is uniq_ref's closed form with
K = e(U - 1).  -S: sdscmp (memcmp, then length).  -C: count descending through glibc's stable qsort over the walk.
"""
import uniq_ref
from uniq_ref import NoAnswer, djb2, epoch


class Result:
    pass


def collapse(data: bytes) -> Result:
    if b"\0" in data:
        raise NoAnswer("NUL byte")
    r = Result()
    r.first, r.members = {}, {}
    r.n = 0
    for name, seq, qual in uniq_ref.records(data):
        if seq not in r.first:
            r.first[seq] = len(r.first)
            r.members[seq] = []
        r.members[seq].append((name, qual))
        r.n += 1
    U = r.u = len(r.first)
    S, K = 0, 0
    if U:
        S = 4
        while S < U:
            S *= 2
        K = epoch(U - 1)
    r.hash_size = S

    def place(key):
        j = r.first[key]
        p = (K - epoch(j)) & 1
        return (djb2(key) & (S - 1), p, j if p else -j)

    r.table_order = sorted(r.first, key=place)
    r.key_order = sorted(r.first)
    r.count_order = sorted(r.table_order, key=lambda k: -len(r.members[k]))   # (sorted() is stable)
    r.max_count = max((len(m) for m in r.members.values()), default=0)
    return r


def render(r: Result, keys) -> bytes:
    out = []
    for k in keys:
        m = r.members[k]
        out.append(b"%s\t%d\n%s\n+\n" % (m[-1][0], len(m), k))
        out.extend(q + b"\n" for _, q in reversed(m))
    return b"".join(out)


def stderr_text(r: Result) -> str:
    pct = "-nan" if r.n == 0 else "%.3f" % (100.0 * r.u / r.n)
    return ("unique reads number = %d(%d / %d = %s%%)\nhash size: %d\nFinished load hash at T s\nFinished  at T s\n"
            % (r.u, r.u, r.n, pct, r.hash_size))


def simulate(data: bytes, by_count=False):
    """The whole tool: (output bytes, stderr as latin-1 text with the run times as 'T', the table)."""
    r = collapse(data)
    return render(r, r.count_order if by_count else r.key_order), stderr_text(r), r
