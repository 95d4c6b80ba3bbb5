"""Python restatement of gzfastq_uniq_sort: framing (uniq_ref.py's), the table's size, the order of the output, the split of
the joined key at strLen, the pair stop and the stderr text.

Held to the recorded reference outputs by test_usort_golden.py; the GPU tests then use it as the checker for random inputs.
Where the reference has no answer `uniq_ref.NoAnswer` is raised.

The order in closed form.  count_read counts e = the groups of four gzgets over mate 1 -- an open line behind the last record
counts --, the table gets S = (size_t)(1.34 * e) slots and is never resized (hashtbl_insert would at count >= 0.75 S, which U <= e
cannot reach).  A new key goes to the head of its chain, dump_hash_table walks slot 0 .. S - 1 and every chain head to tail, and
glibc's qsort (a merge sort: stable) orders that array by count descending.  So the keys come ascending in

    (-count, djb2_64(key) % S, -(ordinal of the key's first record))

with djb2 over 64 bits (hashtbl.c: HSIZE is size_t).  strLen is the length of the first mate-1 sequence that is not empty
(`if (! *strLen)`, set in front of the pair test); mate 1 prints key[:strLen], mate 2 key[strLen:].
"""
import numpy as np

from uniq_ref import NoAnswer, _Gz, records


def djb2_64(key: bytes) -> int:
    h = 5381
    for c in key:
        h = (h * 33 + c) & 0xFFFFFFFFFFFFFFFF
    return h


def count_read(data: bytes) -> int:
    gz, e = _Gz(data), 0
    while gz.gets() is not None:
        gz.gets(), gz.gets(), gz.gets()
        e += 1
    return e


class Result:
    pass


def collapse(data1: bytes, data2: bytes = None) -> Result:
    """The table after load_fastq_file, and the order of qsort_output_hash."""
    r = Result()
    r.paired = data2 is not None
    r.e = count_read(data1)
    r.hash_size = int(1.34 * r.e)
    r.first, r.count, r.error, r.seq_len, r.n, r.loaded = {}, {}, None, 0, 0, []
    it1 = records(data1)
    it2 = records(data2) if r.paired else None
    for i, rec1 in enumerate(it1):
        if not r.seq_len:
            r.seq_len = len(rec1[1])
        key = rec1[1]
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
            key += rec2[1]
            if len(key) > 1023:
                raise NoAnswer("joined key of more than 1023 bytes")
        if key not in r.first:
            r.first[key], r.count[key] = (i, rec1, rec2 if r.paired else None), 1
        else:
            r.count[key] += 1
        r.n += 1
        if r.e // 10 == 0:
            raise NoAnswer("total_reads_count % (elecnt / 10) with fewer than ten reads")
        if r.n % (r.e // 10) == 0:
            r.loaded.append(r.n)
    r.u = len(r.first)
    if r.paired and any(len(k) < r.seq_len for k in r.first):
        raise NoAnswer("key + strLen points behind a key")
    S = r.hash_size
    r.order = sorted(r.first, key=lambda k: (-r.count[k], djb2_64(k) % S, -r.first[k][0]))
    r.max_count = max(r.count.values(), default=0)
    return r


def render(r: Result, mate=0) -> bytes:
    out = []
    for k in r.order:
        name, _, qual = r.first[k][1 + mate]
        out.append(b"%s\t%d\n%s\n+\n%s\n" % (name, r.count[k], k[r.seq_len:] if mate else k[:r.seq_len], qual))
    return b"".join(out)


def stderr_text(r: Result, name1: str, name2: str = None) -> str:
    err = name1 + ("\t" + name2 if name2 is not None else "") + "\n"
    err += "total_reads_num: %d\n" % r.e
    err += "".join("loaded %d at T s\n" % n for n in r.loaded)
    if r.error:
        err += "error at %d: %s\n" % (r.error[0], r.error[1].decode("latin-1"))
    err += "unique reads number = %d\nFinished load hash at T s\nhash size: %d\ntotal reads = %d\n" % (r.u, r.hash_size, r.n)
    pct = "-nan" if r.n == 0 else "%.3f" % float(np.float32(r.u) / np.float32(r.n) * np.float32(100))
    return err + "unique reads percentage: %s%%\nFinished  at T s\n" % pct


def simulate(data1: bytes, data2: bytes = None, name1="r1.fq", name2=None):
    """The whole tool: ({output suffix: bytes after gunzip}, stderr as latin-1 text with the run times as 'T', table)."""
    r = collapse(data1, data2)
    out = {"_1_uniq.fq.gz": render(r, 0)}
    if r.paired:
        out["_2_uniq.fq.gz"] = render(r, 1)
    return out, stderr_text(r, name1, name2 if r.paired else None), r
