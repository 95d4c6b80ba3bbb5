"""What `samtools merge` of samtools-0.1.19 makes of its input files, restated sequentially: the heap's key, the heap itself
(ks_heapmake / ks_heapadjust over one entry per file) with its early end at HEAP_EMPTY, the header rule with its messages, -h,
the level rule, -r's edit of the aux fields, -n, the writer's cuts and zlib at the level the writer was opened with.  The recorded
runs of tests/golden/bammerge/manifest.json pin it to the compiled reference (tests/test_bammerge_golden.py); the tool's host
route (csrc/host/bam_merge_host.hpp) and the device route are held to the same recordings.

merge(files, names, ...) -> (output bytes or None, stderr text, status).  route(files, opts) says which of the tool's routes a
run takes.  effective_order(keys per file) is the device's formulation: a stable sort by the running maximum."""
import struct

import numpy as np

from bai_ref import EOF_BLOCK
from bamsort_ref import MSG_TRUNCATED, cut, fields, header_bytes, member, parse, strnum_cmp

EMPTY = (1 << 64) - 1
USAGE = ("\nUsage:   samtools merge [-nr] [-h inh.sam] <out.bam> <in1.bam> <in2.bam> [...]\n\n"
         "Options: -n       sort by read names\n"
         "         -r       attach RG tag (inferred from file names)\n"
         "         -u       uncompressed BAM output\n"
         "         -f       overwrite the output BAM if exist\n"
         "         -1       compress level 1\n"
         "         -l INT   compression level, from 0 to 9 [-1]\n"
         "         -@ INT   number of BAM compression threads [0]\n"
         "         -R STR   merge file in the specified region STR [all]\n"
         "         -h FILE  copy the header in FILE to <out.bam> [in1.bam]\n\n"
         "Note: Samtools' merge does not reconstruct the @RG dictionary in the header. Users\n"
         "      must provide the correct header with -h, or uses Picard which properly maintains\n"
         "      the header dictionary in merging.\n\n")
MSG_EXISTS = "[bam_merge] File '%s' exists. Please apply '-f' to overwrite. Abort.\n"
MSG_NAME = "[bam_merge_core] different target sequence name: '%s' != '%s' in file '%s'\n"
MSG_OPEN = "open: No such file or directory\n[bam_merge_core] fail to open file %s\n"
MSG_H_OPEN = "[bam_merge_core] cannot open '%s': No such file or directory\n"
MSG_H_COUNT = "[bam_merge_core] number of @SQ headers in '%s' differs from number of target sequences\n"
MSG_H_NAME = "[bam_merge_core] @SQ header '%s' in '%s' differs from target sequence\n"


def key(r):
    """(uint64_t)tid << 32 | (uint32_t)(pos + 1) << 1 | strand of an encoded record"""
    tid, pos, flag = fields(r)
    return ((tid << 32) & EMPTY) | (((pos + 1) << 1) & 0xffffffff) | (flag >> 4 & 1)


def heap_order(keys, by=None):
    """keys: per file the list of its records' keys.  -> [(file, index)] in the order the heap writes them, ending where the top's
    key is EMPTY.  by(file, index) -> (name, flag & 0xc0) switches the comparison to -n's."""
    n = len(keys)
    nxt = [0] * n
    counter = [0]
    heap = [[i, EMPTY, 0, None] for i in range(n)]      # file, key, idx, index of the record at hand (None: the file is used up)

    def refill(e):
        i = e[0]
        if nxt[i] < len(keys[i]):
            e[1], e[2], e[3] = keys[i][nxt[i]], counter[0], nxt[i]
            nxt[i] += 1
            counter[0] += 1
        else:
            e[1], e[3] = EMPTY, None

    def lt(a, b):
        if by is not None:
            if a[3] is None or b[3] is None:
                return a[3] is None
            (na, fa), (nb, fb) = by(a[0], a[3]), by(b[0], b[3])
            t = strnum_cmp(na, nb)
            return t > 0 or (t == 0 and fa > fb)
        return (a[1], a[0], a[2]) > (b[1], b[0], b[2])

    def adjust(i):
        k, tmp = i, heap[i]
        while True:
            k = (k << 1) + 1
            if k >= n:
                break
            if k != n - 1 and lt(heap[k], heap[k + 1]):
                k += 1
            if lt(heap[k], tmp):
                break
            heap[i] = heap[k]
            i = k
        heap[i] = tmp

    for e in heap:
        refill(e)
    for i in range((n >> 1) - 1, -1, -1):
        adjust(i)
    out = []
    while heap[0][1] != EMPTY:
        out.append((heap[0][0], heap[0][3]))
        refill(heap[0])
        adjust(0)
    return out


def effective_keys(keys):
    """per file the running maximum of its keys"""
    return [list(np.maximum.accumulate(np.array(k, np.uint64))) if len(k) else [] for k in keys]


def effective_order(keys):
    """-> ([(file, index)] by a stable sort of the records, file after file, by their effective key; the number of records whose
    effective key is not their own)"""
    flat = [(f, i) for f, k in enumerate(keys) for i in range(len(k))]
    eff = [int(e) for k in effective_keys(keys) for e in k]
    own = [int(x) for k in keys for x in k]
    order = sorted(range(len(flat)), key=lambda j: eff[j])
    return [flat[j] for j in order], sum(1 for a, b in zip(eff, own) if a != b)


def sam_header(text):
    """-h FILE as sam_header_read takes it: (the leading '@' lines, the @SQ lines' SN values)"""
    out, sq, at = b"", [], 0
    while at < len(text) and text[at:at + 1] == b"@":
        e = text.index(b"\n", at)
        line = text[at:e]
        out += line + b"\n"
        if line.startswith(b"@SQ\t"):
            for fld in line.split(b"\t")[1:]:
                if fld.startswith(b"SN:"):
                    sq.append(fld[3:])
                    break
        at = e + 1
    return out, sq


def rg_edit(r, name):
    """bam_aux_get("RG") + bam_aux_del, then bam_aux_append("RG", 'Z', name)"""
    l_qname, n_cigar = r[12], r[16] | r[17] << 8
    l_qseq, = struct.unpack_from("<i", r, 20)
    s = 36 + l_qname + 4 * n_cigar + (l_qseq + 1) // 2 + l_qseq
    width = {"C": 1, "A": 1, "S": 2, "I": 4, "F": 4}
    while s < len(r):
        tag, s = r[s:s + 2], s + 2
        beg = s - 2
        t = chr(r[s]).upper()
        s += 1
        if t in "ZH":
            s = r.index(b"\0", s) + 1
        elif t == "B":
            cnt, = struct.unpack_from("<i", r, s + 1)
            s += 5 + width.get(chr(r[s]).upper(), 0) * cnt
        else:
            s += width.get(t, 0)
        if tag == b"RG":
            r = r[:beg] + r[s:]
            break
    r = r + b"RGZ" + name + b"\0"
    return struct.pack("<i", len(r) - 4) + r[4:]


def rg_name(fn):
    if len(fn) > 4 and fn.endswith(".bam"):
        fn = fn[:-4]
    return fn.rsplit("/", 1)[-1].encode()


def level_of(uncomp=False, level1=False, level=-1):
    """bam_merge_core2 works the mode string out -- -u gives "w0", else -1 gives "w1", else -l INT, 9 for 9 and more, plain "w" below
    0 -- and then opens the output with the literal "w": every option leaves the writer at the default level"""
    return -1


def merge(files, names, by_name=False, rg=False, uncomp=False, level1=False, level=-1, h_name=None, h_text=None):
    """files: the inputs' bytes (None: the file does not exist), names: their names on the command line; h_name / h_text: -h's
    argument and the file's bytes (None: it does not exist).  -> (the output file's bytes or None, stderr, status)"""
    err = ""
    if h_name is not None and h_text is None:
        return None, MSG_H_OPEN % h_name, 1
    text, targets, recs = None, None, []
    for i, data in enumerate(files):
        if data is None:
            return None, err + MSG_OPEN % names[i], 1
        p = parse(data)
        assert p.ok and MSG_TRUNCATED not in p.err, "outside the restatement"
        err += p.err
        recs.append(p.recs)
        if i == 0:
            text, targets = p.text, p.targets
            continue
        for (a, _), (b, _) in zip(targets, p.targets):
            if a != b:
                return None, err + MSG_NAME % (a.decode(), b.decode(), names[i]), 1
        if len(p.targets) > len(targets):
            targets = p.targets
    if h_name is not None:
        h, sq = sam_header(h_text)
        if sq:
            if len(sq) != len(targets):
                return None, err + MSG_H_COUNT % h_name, 1
            for (a, _), b in zip(targets, sq):
                if a != b:
                    return None, err + MSG_H_NAME % (b.decode(), h_name), 1
        text = h
    keys = [[key(r) for r in f] for f in recs]
    by = None
    if by_name:
        assert all(recs), "the reference compares a null name"
        by = lambda f, i: (recs[f][i][36:].split(b"\0")[0], fields(recs[f][i])[2] & 0xc0)
    out = [rg_edit(recs[f][i], rg_name(names[f])) if rg else recs[f][i] for f, i in heap_order(keys, by)]
    lvl = level_of(uncomp, level1, level)
    return b"".join(member(b, lvl) for b in cut(header_bytes(text, targets), out)) + EOF_BLOCK, err, 0


def options(opts):
    """merge()'s arguments of a command line's options (-h's file is the caller's to read)"""
    kw, it = {}, iter(x for o in opts for x in (["-" + ch for ch in o[1:]] if o[0] == "-" and len(o) > 2 and set(o[1:]) <= set("nru1f") else [o]))
    for o in it:
        if o == "-n":
            kw["by_name"] = True
        elif o == "-r":
            kw["rg"] = True
        elif o == "-u":
            kw["uncomp"] = True
        elif o == "-1":
            kw["level1"] = True
        elif o == "-l":
            kw["level"] = int(next(it))
        elif o == "-h":
            kw["h_name"] = next(it)
        elif o == "-@":
            next(it)
    return kw


def route(files, opts):
    """'device' where the header rule lets the run go on, neither -n nor -r is given, no record has the HEAP_EMPTY key and the
    record index's proof takes every file (it refuses a refID, a pos, a mate's refID or a mate's pos below -1 as no record at all:
    a pos of -2 has its key, but never reaches the session);
    else 'host'"""
    kw = options(opts)
    if kw.get("by_name") or kw.get("rg") or any(f is None for f in files):
        return "host"
    for data in files:
        p = parse(data)
        if not p.ok or MSG_TRUNCATED in p.err:
            return "host"
        for r in p.recs:
            tid, pos, _ = fields(r)
            mtid, mpos = struct.unpack_from("<ii", r, 24)
            if key(r) == EMPTY or tid < -1 or pos < -1 or mtid < -1 or mpos < -1:
                return "host"
    return "device"
