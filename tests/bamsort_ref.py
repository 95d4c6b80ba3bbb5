"""What `samtools sort` of samtools-0.1.19 makes of a BAM file, restated sequentially: the key of the in-memory sort and the key of
the merge heap, the stable order, the SO field of the header, the chunk accounting that decides between one block and a merge
(and with it the "merging from N files" message and the level of the output), the merge itself, the writer's cuts and zlib at
the level the writer was opened with.  The recorded runs of tests/golden/bamsort/manifest.json pin it to the compiled reference
(tests/test_bamsort_golden.py); the tool's host route (csrc/host/bam_sort_host.hpp) and the device route are held to the same
recordings.

sort(data, ...) -> (output bytes or None, stderr text).  route(data) says which of the tool's routes a file takes."""
import struct
import zlib

import numpy as np

from bai_ref import Bgzf, EOF_BLOCK, MSG_NO_EOF

FULL = 0xff00
MSG_TRUNCATED = "[bam_sort_core] truncated file. Continue anyway.\n"
MSG_MERGING = "[bam_sort_core] merging from %d files...\n"
USAGE = ("\nUsage:   samtools sort [options] <in.bam> <out.prefix>\n\n"
         "Options: -n        sort by read name\n"
         "         -f        use <out.prefix> as full file name instead of prefix\n"
         "         -o        final output to stdout\n"
         "         -l INT    compression level, from 0 to 9 [-1]\n"
         "         -@ INT    number of sorting and compression threads [1]\n"
         "         -m INT    max memory per thread; suffix K/M/G recognized [768M]\n\n")
DEFAULT_MEM = 768 << 20
POS_MIN, POS_MAX = -1, (1 << 30) - 2      # the device route's domain


def change_so(text, so):
    """bytes -> bytes.  The C string functions see the text up to its first NUL."""
    t = text.split(b"\0")[0]
    beg = end = None
    if len(text) > 3 and t[:3] == b"@HD":
        p = t.find(b"\n")
        if p < 0:
            return text
        q = t[:p].find(b"\tSO:")
        if q >= 0:
            rest = t[q + 4:p]                              # strncmp(q + 4, so, p - q - 4): equal as far as the rest of the line reaches
            if rest == (so + b"\0")[:len(rest)]:
                return text
            e = q + 4
            while t[e] not in b"\n\t":
                e += 1
            beg, end = q, e
        else:
            beg = end = p
    if beg is None:
        return b"@HD\tVN:1.3\tSO:" + so + b"\n" + text
    return text[:beg] + b"\tSO:" + so + text[end:]


def roundup32(x):
    x = (x - 1) & 0xffffffff
    for s in (1, 2, 4, 8, 16):
        x |= x >> s
    return (x + 1) & 0xffffffff


def fresh_mem(sizes):
    """what the reference counts for the records if each comes into a fresh slot"""
    return sum(72 + roundup32(s - 36) for s in sizes)


def plan_chunks(sizes, max_mem, n_threads, sort_part):
    """The reference's temporary files: lists of record ordinals, each in its sorted order; [] when it sorts in one block.
    sort_part(ordinals) -> the same in sorted order.  The buffer's slots keep their capacity from chunk to chunk, and the sort
    moves the slots with their records: slot j of the next chunk has the capacity of the record sorted to place j."""
    files, cap, mem, k, start = [], [], 0, 0, 0

    def close(count):
        nt = max(1, n_threads)
        if count < nt * 64:
            nt = 1
        rest, at = count, 0
        for i in range(nt):
            n = rest // (nt - i)
            part = sort_part(list(range(start + at, start + at + n)))
            cap[at:at + n] = [cap[r - start] for r in part]
            files.append(part)
            rest, at = rest - n, at + n

    for r, s in enumerate(sizes):
        d = s - 36
        if k == len(cap):
            cap.append(0)
        if cap[k] < d:
            cap[k] = roundup32(d)
        if d < cap[k] >> 2:
            cap[k] = roundup32(d)
        mem += 56 + cap[k] + 16
        k += 1
        if mem >= max_mem:
            close(k)
            mem, k, start = 0, 0, r + 1
    if files:
        close(k)
    return files


def keys(tid, pos, flag):
    """(bam1_lt's key, the merge heap's key) as unsigned 64-bit numbers"""
    low = ((pos + 1) << 1) & 0xffffffff
    signed = low - (1 << 32) if low & 0x80000000 else low
    strand = flag >> 4 & 1
    return ((tid << 32) | signed | strand) & (1 << 64) - 1, (((tid << 32) & (1 << 64) - 1) | low | strand)


def strnum_cmp(a, b):
    a, b = a + b"\0", b + b"\0"
    pa = pb = 0
    dig = lambda c: 48 <= c <= 57
    while a[pa] and b[pb]:
        if dig(a[pa]) and dig(b[pb]):
            while a[pa] == 48:
                pa += 1
            while b[pb] == 48:
                pb += 1
            while dig(a[pa]) and dig(b[pb]) and a[pa] == b[pb]:
                pa, pb = pa + 1, pb + 1
            if dig(a[pa]) and dig(b[pb]):
                i = 0
                while dig(a[pa + i]) and dig(b[pb + i]):
                    i += 1
                return 1 if dig(a[pa + i]) else -1 if dig(b[pb + i]) else a[pa] - b[pb]
            if dig(a[pa]):
                return 1
            if dig(b[pb]):
                return -1
            if pa != pb:
                return 1 if pa < pb else -1
        else:
            if a[pa] != b[pb]:
                return a[pa] - b[pb]
            pa, pb = pa + 1, pb + 1
    return 1 if a[pa] else -1 if b[pb] else 0


class Parsed:
    def __init__(self):
        self.err = ""
        self.text = b""
        self.targets = []        # (name as a C string, length)
        self.recs = []           # whole records, 4 + block_size bytes
        self.ok = False


def parse(data):
    """the file as bam_header_read and bam_read1 take it"""
    p = Parsed()
    if data[-28:] != EOF_BLOCK:
        p.err += MSG_NO_EOF
    z = Bgzf(data)
    magic = z.read(4)
    if magic != b"BAM\1":
        return p
    l_text, = struct.unpack("<i", z.read(4))
    p.text = z.read(l_text)
    n_ref, = struct.unpack("<i", z.read(4))
    for _ in range(n_ref):
        l_name, = struct.unpack("<i", z.read(4))
        name = z.read(l_name)
        ln, = struct.unpack("<i", z.read(4))
        p.targets.append((name.split(b"\0")[0], ln))
    p.ok = True
    while True:
        w = z.read(4)
        if w is None or len(w) != 4:
            status = -1 if w == b"" else -2
            break
        block_len, = struct.unpack("<i", w)
        x = z.read(32)
        if x is None or len(x) != 32:
            status = -3
            break
        d = z.read(block_len - 32)
        if block_len < 32 or d is None or len(d) != block_len - 32:
            status = -4
            break
        p.recs.append(w + x + d)
    if status != -1:
        p.err += MSG_TRUNCATED
    return p


def fields(r):
    tid, pos, _, flag_nc = struct.unpack_from("<iiII", r, 4)
    return tid, pos, flag_nc >> 16


def route(data):
    """'device' where every record has -1 <= pos <= 2^30 - 2, the file is whole and the record index's proof takes it (it refuses a
    refID, a mate's refID or a mate's pos below -1 as no record at all); else 'host'"""
    p = parse(data)
    if not p.ok or MSG_TRUNCATED in p.err:
        return "host"
    for r in p.recs:
        tid, pos, _ = fields(r)
        mtid, mpos = struct.unpack_from("<ii", r, 24)
        if not POS_MIN <= pos <= POS_MAX or tid < -1 or mtid < -1 or mpos < -1:
            return "host"
    return "device"


def model_keys(recs):
    """bam1_lt's keys as a numpy array, for the order tests"""
    return np.array([keys(*fields(r))[0] for r in recs], np.uint64)


def order_of(recs, by_name, max_mem, n_threads):
    """-> (indices into recs in output order, number of temporary files)"""
    def lt_key(i):
        return keys(*fields(recs[i]))[0]

    def name(i):
        return recs[i][36:].split(b"\0")[0]

    def sort_part(idx):
        if not by_name:
            return sorted(idx, key=lt_key)
        import functools
        return sorted(idx, key=functools.cmp_to_key(
            lambda a, b: strnum_cmp(name(a), name(b)) or ((fields(recs[a])[2] & 0xc0) - (fields(recs[b])[2] & 0xc0))))

    files = plan_chunks([len(r) for r in recs], max_mem, n_threads, sort_part)
    if not files:
        return sort_part(list(range(len(recs)))), 0
    # the heap of the merge: ks_heapmake / ks_heapadjust over one entry per file
    EMPTY = (1 << 64) - 1
    nxt = [0] * len(files)
    counter = [0]

    def refill(e):
        i = e[0]
        if nxt[i] < len(files[i]):
            r = files[i][nxt[i]]
            nxt[i] += 1
            e[1], e[2], e[3] = keys(*fields(recs[r]))[1], counter[0], r
            counter[0] += 1
        else:
            e[1], e[3] = EMPTY, None

    def heap_lt(a, b):
        if by_name:
            if a[3] is None or b[3] is None:
                return a[3] is None
            t = strnum_cmp(name(a[3]), name(b[3]))
            return t > 0 or (t == 0 and (fields(recs[a[3]])[2] & 0xc0) > (fields(recs[b[3]])[2] & 0xc0))
        return (a[1], a[0], a[2]) > (b[1], b[0], b[2])

    heap = [[i, EMPTY, 0, None] for i in range(len(files))]
    for e in heap:
        refill(e)
    n = len(heap)

    def adjust(i):
        k, tmp = i, heap[i]
        while True:
            k = (k << 1) + 1
            if k >= n:
                break
            if k != n - 1 and heap_lt(heap[k], heap[k + 1]):
                k += 1
            if heap_lt(heap[k], tmp):
                break
            heap[i] = heap[k]
            i = k
        heap[i] = tmp

    for i in range((n >> 1) - 1, -1, -1):
        adjust(i)
    out = []
    while heap[0][1] != EMPTY:
        out.append(heap[0][3])
        refill(heap[0])
        adjust(0)
    return out, len(files)


def header_bytes(text, targets):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(targets))
    for name, ln in targets:
        h += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return h


def cut(hdr, recs):
    """the writer's blocks: the header in blocks of its own, then bam_write1's rule"""
    out = [hdr[i:i + FULL] for i in range(0, len(hdr), FULL)]
    cur = b""
    for r in recs:
        if len(cur) + len(r) > FULL and cur:
            out.append(cur)
            cur = b""
        while r:
            k = min(FULL - len(cur), len(r))
            cur, r = cur + r[:k], r[k:]
            if len(cur) == FULL:
                out.append(cur)
                cur = b""
    if cur:
        out.append(cur)
    return out


def member(piece, level):
    """one block as bgzf.c's deflate_block makes it: deflate() in ONE Z_FINISH call -- at level 0 that is one final stored block,
    01 LEN NLEN (compressobj's compress() + flush() are two calls and end with an empty stored block of their own)"""
    if level == 0:
        comp = b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) + piece
    else:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
        comp = co.compress(piece) + co.flush()
    return (struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece)))


def sort(data, by_name=False, level=-1, n_threads=0, max_mem=DEFAULT_MEM):
    """-> (the output file's bytes, stderr)"""
    p = parse(data)
    assert p.ok
    nt = 1 if n_threads < 2 else n_threads
    order, n_files = order_of(p.recs, by_name, max_mem * nt, nt)
    err = p.err
    lvl = -1 if level < 0 else min(level, 9)
    if n_files:
        err += MSG_MERGING % n_files
        lvl = -1
    text = change_so(p.text, b"queryname" if by_name else b"coordinate")
    blocks = cut(header_bytes(text, p.targets), [p.recs[i] for i in order])
    return b"".join(member(b, lvl) for b in blocks) + EOF_BLOCK, err


def options(opts):
    """sort()'s arguments of a command line's options"""
    kw, it = {}, iter(opts)
    for o in it:
        if o == "-n":
            kw["by_name"] = True
        elif o == "-l":
            kw["level"] = int(next(it))
        elif o == "-@":
            kw["n_threads"] = int(next(it))
        elif o == "-m":
            v = next(it)
            kw["max_mem"] = int(v[:-1]) << 10 if v[-1] in "kK" else int(v)
    return kw


def sorted_stream(data):
    """the sorted records of a file inside the device's domain, for the ABI tests: (records in output order, order)"""
    p = parse(data)
    order = list(np.argsort(model_keys(p.recs), kind="stable")) if p.recs else []
    return [p.recs[i] for i in order], order
