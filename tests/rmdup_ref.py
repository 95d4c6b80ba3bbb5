"""What `samtools rmdup` of samtools-0.1.19 makes of a BAM file, restated sequentially: bam_rmdup_core (pairs) and bam_rmdupse_core
(-s / -S) record by record with their tables -- the library of a record (the header's @RG lines as sam_header_parse2 and
sam_header2tbl read them, the RG tag as bam_aux_get finds it), best_hash with its 0x40000 rule, the stack, the set of names, the
SE queue on its recycled list nodes -- the library lines in khash's iteration order, and the writer of samopen(.., "wb", ..).
The recorded runs of tests/golden/rmdup/manifest.json pin it to the compiled reference (tests/test_rmdup_golden.py); the tool's
host route (csrc/host/bam_rmdup_host.hpp) and the device route are held to the same recordings.

rmdup(data, se, force_se) -> (output bytes, stderr text, order).  Undefined is raised where the reference reads memory that is
not its own (a hit on a stale best_hash key, an aux walk or a name past its record, a refID the header does not have).

The second half is what the device route computes instead of the name set: neighbour_rule() against sequential_set()
(docs/kernels/bam_rmdup.md has the derivation), and plan(), the whole paired core as sorts, group walks and scans."""
import struct

from bai_ref import EOF_BLOCK, MSG_NO_EOF, calend
from bamsort_ref import cut, header_bytes, member, parse

USAGE = ("\nUsage:  samtools rmdup [-sS] <input.srt.bam> <output.bam>\n\n"
         "Option: -s    rmdup for SE reads\n"
         "        -S    treat PE reads as SE in rmdup (force -s)\n\n")
BUFFER_SIZE = 0x40000
QUEUE_CLEAR_SIZE = 0x100000
MAX_POS = 0x7fffffff
PRIMES = [0, 3, 11, 23, 53, 97, 193, 389, 769, 1543, 3079, 6151, 12289, 24593, 49157, 98317, 196613, 393241, 786433, 1572869, 3145739, 6291469,
          12582917, 25165843, 50331653, 100663319, 201326611, 402653189, 805306457, 1610612741, 3221225473, 4294967291]


class Undefined(Exception):
    pass


# ---- a record's fields ----------------------------------------------------------------------------------------------------------------

class Rec:
    __slots__ = ("b", "tid", "pos", "l_qname", "n_cigar", "flag", "l_qseq", "mtid", "isize")

    def __init__(self, b):
        self.b = b
        self.tid, self.pos, bmn, fnc, self.l_qseq, self.mtid, _, self.isize = struct.unpack_from("<iiIIiiii", b, 4)
        self.l_qname, self.n_cigar, self.flag = bmn & 0xff, fnc & 0xffff, fnc >> 16

    def name(self):
        """bam1_qname as a C string"""
        end = self.b.find(b"\0", 36)
        if end < 0:
            raise Undefined("a read name runs past its record")
        return self.b[36:end]

    def cigar(self):
        at = 36 + self.l_qname
        if at + 4 * self.n_cigar > len(self.b):
            raise Undefined("a CIGAR runs past its record")
        return list(struct.unpack_from("<%dI" % self.n_cigar, self.b, at))

    def sum_qual(self):
        at = 36 + self.l_qname + 4 * self.n_cigar + (self.l_qseq + 1) // 2
        if self.l_qseq < 0:
            return 0
        if at + self.l_qseq > len(self.b):
            raise Undefined("the qualities run past their record")
        return sum(self.b[at:at + self.l_qseq])

    def aux_get(self, tag):
        """bam_aux_get: the offset of the field's type byte, or None.  __skip_tag upper-cases the type before it looks up the size,
        so `d` has size 0 like every type it does not know; a B array's subtype is looked up as it is."""
        b, end = self.b, len(self.b)
        s = 36 + self.l_qname + 4 * self.n_cigar + (self.l_qseq + 1) // 2 + self.l_qseq
        size = {67: 1, 99: 1, 65: 1, 83: 2, 115: 2, 73: 4, 105: 4, 102: 4, 70: 4}
        try:
            while s < end:
                x = bytes((b[s], b[s + 1]))
                s += 2
                if x == tag:
                    return s
                t = b[s]
                t = t - 32 if 97 <= t <= 122 else t
                s += 1
                if t in (90, 72):
                    while b[s]:
                        s += 1
                    s += 1
                elif t == 66:
                    s += 5 + size.get(b[s], 0) * struct.unpack_from("<i", b, s + 1)[0]
                else:
                    s += size.get(t, 0)
                if s < 0:
                    raise Undefined("an aux walk leaves its record")
        except (IndexError, struct.error):
            raise Undefined("an aux walk leaves its record")
        return None


# ---- the header's @RG lines -----------------------------------------------------------------------------------------------------------

def header_lines(text, err):
    """sam_header_parse2 -> [(type, [(key, value)])], or None where it gives up (its words go to err)"""
    lines, at = [], 0
    while at < len(text):
        to = at
        while to < len(text) and text[to] not in (10, 13):
            to += 1
        line = text[at:to]
        if to < len(text):
            if text[to] == 10:
                to += 1
            elif text[to:to + 2] == b"\r\n":
                to += 2
            elif to == at:
                raise Undefined("a lone CR in the header: nextline does not move")        # (it loops for ever)
        at = to
        s = line.decode("latin-1")
        if line[:1] != b"@":
            err.append("[sam_header_line_parse] expected '@', got [%s]\n" % s)
            return None
        f = line[1:].split(b"\t")
        if len(f[0]) != 2:
            err.append("[sam_header_line_parse] expected '@XY', got [%s]\nHint: The header tags must be tab-separated.\n" % s)
            return None
        typ = f[0]
        if typ not in (b"HD", b"SQ", b"RG", b"PG", b"CO"):
            raise Undefined("a header line of unknown type: the tag tables are read out of bounds")
        rest = line[3:]
        tabs = len(rest) - len(rest.lstrip(b"\t"))
        if tabs != 1:
            err.append("[sam_header_line_parse] multiple tabs on line [%s] (%d)\n" % (s, tabs))
            return None
        rest = rest[1:]
        tags = []
        if typ == b"CO":
            if rest:
                tags.append((b"  ", rest))
        else:
            p = 0
            while p < len(rest):
                q = rest.find(b"\t", p)
                q = len(rest) if q < 0 else q
                field = rest[p:q]
                if len(field) < 3:
                    raise Undefined("a header tag shorter than XY:")
                if any(k == field[:2] for k, _ in tags):
                    err.append("The tag '%s' present (at least) twice on line [%s]\n" % (field[:2].decode("latin-1"), s))
                tags.append((field[:2], field[3:]))
                r = q
                while r < len(rest) and rest[r] == 9:
                    r += 1
                if r < len(rest) and r - q != 1:
                    err.append("[sam_header_line_parse] multiple tabs on line [%s] (%d)\n" % (s, r - q))
                    return None
                p = r
        lines.append((typ, tags))
    return lines or None


def first_tag(tags, key):
    for k, v in tags:
        if k == key:
            return v
    return None


class Libraries:
    """bam_get_library: the header is parsed on the first call -- and again on every call while parsing fails"""

    def __init__(self, text, err):
        self.text, self.err, self.dict, self.tbl = text.split(b"\0")[0], err, None, None

    def table(self):
        if self.dict is None:
            self.dict = header_lines(self.text, self.err)
        if self.tbl is None:
            self.tbl = {}
            for typ, tags in self.dict or []:
                if typ == b"RG":
                    k, v = first_tag(tags, b"ID"), first_tag(tags, b"LB")
                    if k is not None and v is not None:
                        if k in self.tbl:
                            self.err.append("[sam_header_lookup_table] They key %s not unique.\n" % k.decode("latin-1"))
                        self.tbl[k] = v
        return self.tbl

    def of(self, rec):
        self.table()
        rg = rec.aux_get(b"RG")
        if rg is None:
            return b"\t"
        end = rec.b.find(b"\0", rg + 1)
        if end < 0:
            raise Undefined("an RG value runs past its record")
        return self.tbl.get(rec.b[rg + 1:end], b"\t")


def id_table(text):
    """{ID: library} as the device route is given it, or None where the header is not parsed in silence"""
    err = []
    try:
        tbl = Libraries(text, err).table()
    except Undefined:
        return None
    return None if err else tbl


# ---- khash's order over strings ---------------------------------------------------------------------------------------------------------

def x31(s):
    h = 0
    for k, c in enumerate(s):
        c = c - 256 if c >= 128 else c
        h = c & 0xffffffff if k == 0 else (h * 31 + c) & 0xffffffff
    return h


class KhStrings:
    """the bucket order of a khash 0.2.5 string table that only grows (kh_put, kh_resize)"""

    def __init__(self):
        self.nb, self.size, self.upper, self.keys = 0, 0, 0, []

    def _resize(self, want):
        t = len(PRIMES) - 1
        while PRIMES[t] > want:
            t -= 1
        nb = PRIMES[t + 1]
        if self.size >= int(nb * 0.77 + 0.5):
            return
        new, old = [None] * nb, self.keys + [None] * max(0, nb - self.nb)
        moved = [k is None for k in old]
        for j in range(self.nb):
            if moved[j]:
                continue
            key, moved[j] = old[j], True
            while True:
                k = x31(key)
                i, inc = k % nb, 1 + k % (nb - 1)
                while new[i] is not None:
                    i = i + inc - nb if i + inc >= nb else i + inc
                new[i] = True
                if i < self.nb and not moved[i]:
                    old[i], key = key, old[i]
                    moved[i] = True
                else:
                    old[i] = key
                    break
        self.keys = [old[i] if new[i] else None for i in range(nb)]
        self.nb, self.upper = nb, int(nb * 0.77 + 0.5)

    def put(self, key):
        if key in self.keys:
            return
        if self.size >= self.upper:
            self._resize(self.nb - 1 if self.nb > self.size << 1 else self.nb + 1)
        k = x31(key)
        i, inc = k % self.nb, 1 + k % (self.nb - 1)
        while self.keys[i] is not None:
            i = i + inc - self.nb if i + inc >= self.nb else i + inc
        self.keys[i] = key
        self.size += 1

    def order(self):
        return [k for k in self.keys if k is not None]


def library_lines(core, counts, first_seen):
    """counts: {library: [removed, checked]}; first_seen: the libraries in the order their first record came"""
    kh = KhStrings()
    for lib in first_seen:
        kh.put(lib)
    return ["[%s] %d / %d = %.4f in library '%s'\n" % (core, counts[lib][0], counts[lib][1], counts[lib][0] / counts[lib][1], lib.decode("latin-1"))
            for lib in kh.order()]


# ---- the two cores ----------------------------------------------------------------------------------------------------------------------

class Slot:
    __slots__ = ("rec", "written")

    def __init__(self, rec):
        self.rec, self.written = rec, False


def core_pairs(recs, text, targets, err):
    """bam_rmdup_core -> the ordinals of the records it writes, in output order"""
    out, stack, del_set = [], [], set()
    best, counts, seen = {}, {}, []          # library -> {key: Slot}, [removed, checked]
    libs = Libraries(text, err)
    last_tid, last_pos = -1, -1

    def dump():
        for s in stack:
            out.append(s.rec)
            s.written = True
        del stack[:]

    for i, r in enumerate(recs):
        if r.tid != last_tid or r.pos != last_pos:
            dump()
            for h in best.values():
                if len(h) >= BUFFER_SIZE:
                    h.clear()
            if r.tid != last_tid:
                for h in best.values():
                    h.clear()
                if del_set:
                    err.append("[bam_rmdup_core] %d unmatched pairs\n" % len(del_set))
                    del_set.clear()
                if r.tid == -1:
                    out.extend(range(i, len(recs)))
                    break
                last_tid = r.tid
                if not 0 <= r.tid < len(targets):
                    raise Undefined("a refID the header does not have")
                err.append("[bam_rmdup_core] processing reference %s...\n" % targets[r.tid][0].decode("latin-1"))
        if not r.flag & 1 or r.flag & 12 or (r.mtid >= 0 and r.tid != r.mtid):
            out.append(i)
        elif r.isize > 0:
            lib = libs.of(r)
            if lib not in counts:
                counts[lib], best[lib] = [0, 0], {}
                seen.append(lib)
            counts[lib][1] += 1
            key = (r.pos & 0xffffffff) << 32 | r.isize
            s = best[lib].get(key)
            if s is not None:
                if s.written:
                    raise Undefined("a stale best_hash key is hit: the record behind it has been freed")
                counts[lib][0] += 1
                if recs[s.rec].sum_qual() < r.sum_qual():
                    name = recs[s.rec].name()
                    s.rec = i
                else:
                    name = r.name()
                if name in del_set:
                    err.append("[bam_rmdup_core] inconsistent BAM file for pair '%s'. Continue anyway.\n" % r.name().decode("latin-1"))
                del_set.add(name)
            else:
                s = best[lib][key] = Slot(i)
                stack.append(s)
        else:
            name = r.name()
            if name in del_set:
                del_set.discard(name)
            else:
                out.append(i)
        last_pos = r.pos
    dump()
    err.extend(library_lines("bam_rmdup_core", counts, seen))
    return out


class Node:
    __slots__ = ("endpos", "score", "discarded", "rec")


def core_single(recs, text, err, force_se):
    """bam_rmdupse_core.  The queue is a klist: a node that leaves goes to a pool and is the next one taken, and the tables may
    still point at it."""
    out, queue, pool = [], [], []
    head = [0]
    left, right, counts, seen = {}, {}, {}, []
    libs = Libraries(text, err)
    last_tid = -2

    def push(i, endpos, score):
        n = pool.pop() if pool else Node()
        n.endpos, n.score, n.discarded, n.rec = endpos, score & 0x7fffffff, False, i
        queue.append(n)
        return n

    def dump(pos):
        if len(queue) - head[0] > QUEUE_CLEAR_SIZE or pos == MAX_POS:
            while head[0] < len(queue):
                n = queue[head[0]]
                if not n.discarded:
                    if recs[n.rec].flag & 16 and n.endpos > pos:
                        break
                    out.append(n.rec)
                head[0] += 1
                pool.append(n)
            if head[0] > 1 << 16:
                del queue[:head[0]]
                head[0] = 0
            for lib in seen:              # (every table of every library, whatever the order)
                for h in (left[lib], right[lib]):
                    for k in [k for k, n in h.items() if n.endpos <= pos]:
                        del h[k]

    for i, r in enumerate(recs):
        endpos = calend(r.pos, r.cigar()) & 0xffffffff
        endpos = endpos - (1 << 32) if endpos & 0x80000000 else endpos
        score = r.sum_qual()
        if last_tid != r.tid:
            if last_tid >= 0:
                dump(MAX_POS)
            last_tid = r.tid
        else:
            dump(r.pos)
        if r.flag & 4 or (r.flag & 1 and not force_se):
            push(i, endpos, score)
            continue
        lib = libs.of(r)
        if lib not in counts:
            counts[lib], left[lib], right[lib] = [0, 0], {}, {}
            seen.append(lib)
        counts[lib][1] += 1
        rev = bool(r.flag & 16)
        h, key = (right[lib], endpos & 0xffffffff) if rev else (left[lib], r.pos & 0xffffffff)
        n = h.get(key)
        if n is None:
            h[key] = push(i, endpos, score)
            continue
        counts[lib][0] += 1
        if n.score < score:
            if rev:
                n.discarded = True
                h[key] = push(i, endpos, score)
            else:
                n.score, n.endpos, n.rec = score & 0x7fffffff, endpos, i
    dump(MAX_POS)
    err.extend(library_lines("bam_rmdupse_core", counts, seen))
    return out


def rmdup(data, se=False, force_se=False):
    """-> (the output file's bytes, stderr, the input ordinals of the output's records)"""
    p = parse(data)
    assert p.ok
    err = [MSG_NO_EOF] if MSG_NO_EOF in p.err else []
    recs = [Rec(b) for b in p.recs]
    order = core_single(recs, p.text, err, force_se) if se or force_se else core_pairs(recs, p.text, p.targets, err)
    blocks = cut(header_bytes(p.text, p.targets), [p.recs[i] for i in order])
    return b"".join(member(b, -1) for b in blocks) + EOF_BLOCK, "".join(err), order


def options(opts):
    return {"se": "-s" in opts or "-S" in opts, "force_se": "-S" in opts}


# ---- what the device computes instead -----------------------------------------------------------------------------------------------------

R_TID_BACK, R_POS_BACK, R_RECORDS, R_RG_TYPE, R_AUX, R_NAME, R_INCONSISTENT, R_COLLISION, R_FIRST_UNPLACED, R_TID_BEYOND, R_POS_NEG, R_FIELDS = range(1, 13)
KNOWN = set(b"AcCsSiIfZHB")
KNOWN_SUB = set(b"cCsSiIf")


def aux_reason(r):
    """0, or why the device hands a head's aux walk to the host: an RG that is not Z, a type it does not take, a walk past the record"""
    b, end = r.b, len(r.b)
    s = 36 + r.l_qname + 4 * r.n_cigar + (r.l_qseq + 1) // 2 + r.l_qseq
    size = {67: 1, 99: 1, 65: 1, 83: 2, 115: 2, 73: 4, 105: 4, 102: 4}
    if s > end:
        return R_FIELDS
    while s < end:
        if s + 3 > end:
            return R_AUX
        tag, t = b[s:s + 2], b[s + 2]
        s += 3
        if tag == b"RG" and t != 90:
            return R_RG_TYPE
        if t not in KNOWN:
            return R_AUX
        if t in (90, 72):
            e = b.find(b"\0", s)
            if e < 0:
                return R_AUX
            if tag == b"RG":
                return 0
            s = e + 1
        elif t == 66:
            if s + 5 > end or b[s] not in KNOWN_SUB:
                return R_AUX
            n = struct.unpack_from("<i", b, s + 1)[0]
            if n < 0 or s + 5 + size[b[s]] * n > end:
                return R_AUX
            s += 5 + size[b[s]] * n
        else:
            s += size[t]
            if s > end:
                return R_AUX
    return 0


def classify(r):
    """'P' written at once, 'H' head, 'T' tail"""
    if not r.flag & 1 or r.flag & 12 or (r.mtid >= 0 and r.tid != r.mtid):
        return "P"
    return "H" if r.isize > 0 else "T"


def first_refusal(recs, n_targets):
    """(ordinal, reason) of the first record for which the device route's per-record checks send the file to the host, or None.
    (An inconsistent pair is found later, from the sorted events: plan() reports it.)"""
    for i, r in enumerate(recs):
        if i == 0 and r.tid == -1:
            return i, R_FIRST_UNPLACED
        if r.tid == -1:
            continue
        if i and recs[i - 1].tid == -1 or i and (r.tid & 0xffffffff) < (recs[i - 1].tid & 0xffffffff):
            return i, R_TID_BACK
        if r.tid >= n_targets:
            return i, R_TID_BEYOND
        if r.pos < 0:
            return i, R_POS_NEG
        if i and r.tid == recs[i - 1].tid and r.pos < recs[i - 1].pos:
            return i, R_POS_BACK
        c = classify(r)
        if c != "P":
            if r.l_qname == 0 or 36 + r.l_qname > len(r.b) or r.b[36 + r.l_qname - 1] != 0 or 0 in r.b[36:36 + r.l_qname - 1]:
                return i, R_NAME
        if c == "H":
            if r.l_qseq < 0 or 36 + r.l_qname + 4 * r.n_cigar + (r.l_qseq + 1) // 2 + r.l_qseq > len(r.b):
                return i, R_FIELDS
            a = aux_reason(r)
            if a:
                return i, a
    return None


def route(data):
    """'device' where the file is whole, its header is parsed in silence, the record index takes every record (no refID, mate's refID
    or mate's pos below -1) and no record is outside the device's domain; else 'host'"""
    from bamsort_ref import MSG_TRUNCATED
    p = parse(data)
    if not p.ok or MSG_TRUNCATED in p.err:
        return "host"
    tbl = id_table(p.text)
    recs = [Rec(b) for b in p.recs]
    if tbl is None or first_refusal(recs, len(p.targets)) is not None:
        return "host"
    if any(r.tid < -1 or r.mtid < -1 or struct.unpack_from("<i", r.b, 28)[0] < -1 for r in recs):
        return "host"
    return "host" if plan(recs, tbl)[3] is not None else "device"


def sequential_set(events):
    """events in time order: (segment, name, 'I' | 'T').  -> (dropped: the times of the tails that are dropped, inconsistent: the
    times of the insertions that find their name, unmatched: {segment: names left})"""
    dropped, bad, unmatched, names, seg = [], [], {}, set(), None
    for t, (s, name, kind) in enumerate(events):
        if s != seg:
            if names:
                unmatched[seg] = len(names)
            names, seg = set(), s
        if kind == "I":
            if name in names:
                bad.append(t)
            names.add(name)
        elif name in names:
            names.discard(name)
            dropped.append(t)
    if names:
        unmatched[seg] = len(names)
    return dropped, bad, unmatched


def neighbour_rule(events):
    """the same from a stable sort by (segment, name) and one look at the left neighbour"""
    idx = sorted(range(len(events)), key=lambda t: (events[t][0], events[t][1]))
    dropped, bad, unmatched = [], [], {}
    for j, t in enumerate(idx):
        s, name, kind = events[t]
        left = events[idx[j - 1]] if j and events[idx[j - 1]][:2] == (s, name) else None
        if kind == "T" and left is not None and left[2] == "I":
            dropped.append(t)
        if kind == "I" and left is not None and left[2] == "I":
            bad.append(t)
        last = j + 1 == len(idx) or events[idx[j + 1]][:2] != (s, name)
        if kind == "I" and last:
            unmatched[s] = unmatched.get(s, 0) + 1
    return sorted(dropped), sorted(bad), unmatched


def plan(recs, tbl):
    """The paired core inside the device's domain, as the device computes it: runs and segments from the left neighbour, groups by a
    stable sort of the heads, a walk over each group, events at the time of the record being read, the neighbour rule, and the
    output index of every survivor from two counts.  tbl: {ID: library}.
    -> (order, {library: [removed, checked, first ordinal]}, {refID: unmatched}, inconsistent ordinal or None)"""
    n = len(recs)
    cls = ["U" if r.tid == -1 else classify(r) for r in recs]
    run, k = [], -1
    for i, r in enumerate(recs):
        if i == 0 or (r.tid, r.pos) != (recs[i - 1].tid, recs[i - 1].pos) and not (r.tid == -1 and recs[i - 1].tid == -1):
            k += 1
        run.append(k)
    lib_of = {}
    for i, r in enumerate(recs):
        if cls[i] == "H":
            rg = r.aux_get(b"RG")
            lib_of[i] = b"\t" if rg is None else tbl.get(r.b[rg + 1:r.b.find(b"\0", rg + 1)], b"\t")
    heads = sorted((i for i in range(n) if cls[i] == "H"), key=lambda i: (run[i], lib_of[i], recs[i].isize))
    slot, event, counts = {}, {}, {}          # first ordinal -> survivor; time -> (ordinal whose name, 'I' | 'T')
    j = 0
    while j < len(heads):
        e = j
        key = (run[heads[j]], lib_of[heads[j]], recs[heads[j]].isize)
        while e < len(heads) and (run[heads[e]], lib_of[heads[e]], recs[heads[e]].isize) == key:
            e += 1
        holder = heads[j]
        for b in heads[j + 1:e]:
            if recs[holder].sum_qual() < recs[b].sum_qual():
                event[b] = (holder, "I")
                holder = b
            else:
                event[b] = (b, "I")
        slot[heads[j]] = holder
        c = counts.setdefault(key[1], [0, 0, heads[j]])
        c[0], c[1], c[2] = c[0] + e - j - 1, c[1] + e - j, min(c[2], heads[j])
        j = e
    for i in range(n):
        if cls[i] == "T":
            event[i] = (i, "T")
    times = sorted(event)
    ev = [(recs[t].tid, recs[event[t][0]].name(), event[t][1]) for t in times]
    dropped, bad, unmatched = neighbour_rule(ev)
    gone = {times[t] for t in dropped}
    now = [1 if cls[i] in "PU" or (cls[i] == "T" and i not in gone) else 0 for i in range(n)]
    c_now, c_slot = [0], [0]
    for i in range(n):
        c_now.append(c_now[-1] + now[i])
        c_slot.append(c_slot[-1] + (1 if i in slot else 0))
    start, end = {}, {}
    for i in range(n):
        start.setdefault(run[i], i)
        end[run[i]] = i + 1
    order = [None] * (c_now[n] + c_slot[n])
    for i in range(n):
        if now[i]:
            order[c_now[i] + c_slot[start[run[i]]]] = i
        if i in slot:
            order[c_now[end[run[i]]] + c_slot[i]] = slot[i]
    return order, counts, unmatched, (times[bad[0]] if bad else None)
