"""What `samtools fixmate` of samtools-0.1.19 (bam_mate.c) makes of its input, restated sequentially: bam_mating_core's loop with
its one pending record, bam_calend with the backward walk of the B op, the 0x4 update against the target's length, the pair and
singleton fixes, bam_template_cigar's CT field with kputw's digits, the writer's cuts and zlib at the default level.  The recorded
runs of tests/golden/fixmate/manifest.json pin it to the compiled reference (tests/test_fixmate_golden.py); the tool's host route
(csrc/host/bam_fixmate_host.hpp) and the device route are held to the same recordings.

fixmate(data, remove_reads) -> (output bytes or None, stderr text, status).  machine(recs, target_len, remove_reads) is the loop
alone: [(ordinal, the record as written)] and the counts.  closed_form(cls, names, remove_reads) is the device's formulation of the
pairing and the output's order: parity inside runs of equal names, and a scan of what every record makes the reference write.
route(data) says which of the tool's routes a run takes."""
import struct

from bai_ref import EOF_BLOCK, MSG_NO_EOF
from bamsort_ref import cut, header_bytes, member, parse
from bamsort_ref import route as index_route

USAGE = ("Usage: samtools fixmate <in.nameSrt.bam> <out.nameSrt.bam>\n"
         "Options:\n"
         "       -r    remove unmapped reads and secondary alignments\n")
CIGAR_STR = b"MIDNSHP=XB\0"      # BAM_CIGAR_STR with its NUL: op 10 reads it, ops 11..15 read past it
CIGAR_TYPE = 0x3C1A7
LIVE, SKIP_TID, SKIP_SECONDARY = 0, 1, 2
FIRST, SECOND, SINGLE, PENDING, SKIPPED = range(5)


class Undefined(Exception):
    """the reference reads memory that is not its own"""


def core(r):
    tid, pos, bmq, fn, l_seq, mtid, mpos, isize = struct.unpack_from("<iiIIiiii", r, 4)
    return {"tid": tid, "pos": pos, "l_qname": bmq & 0xff, "n_cigar": fn & 0xffff, "flag": fn >> 16, "mtid": mtid, "mpos": mpos, "isize": isize}


def cigar(r):
    c = core(r)
    at = 36 + c["l_qname"]
    if at + 4 * c["n_cigar"] > len(r):
        raise Undefined("a CIGAR runs past its record")
    return list(struct.unpack_from("<%dI" % c["n_cigar"], r, at))


def qname(r):
    """bam1_qname as a C string"""
    e = r.find(b"\0", 36)
    if e < 0:
        raise Undefined("a read name runs past its record")
    return r[36:e]


def ctype(op):
    return CIGAR_TYPE >> (op << 1) & 3


def wrap(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def calend(r):
    """bam_calend, bam.c:17-41"""
    cg, pos = cigar(r), core(r)["pos"]
    end = pos
    for k, c in enumerate(cg):
        op, ln = c & 15, c >> 4
        if op == 9:
            if k == len(cg) - 1:
                break
            u = v = 0
            l = k - 1
            while l >= 0:
                op1, len1 = cg[l] & 15, cg[l] >> 4
                if ctype(op1) & 1:
                    if u + len1 >= ln:
                        if ctype(op1) & 2:
                            v += ln - u
                        break
                    u += len1
                if ctype(op1) & 2:
                    v += len1
                l -= 1
            end = pos if l < 0 else end - v
        elif ctype(op) & 2:
            end += ln
    return wrap(end)


def with_core(r, flag=None, mtid=None, mpos=None, isize=None):
    b = bytearray(r)
    if flag is not None:
        struct.pack_into("<H", b, 18, flag & 0xffff)
    if mtid is not None:
        struct.pack_into("<i", b, 24, mtid)
    if mpos is not None:
        struct.pack_into("<i", b, 28, mpos)
    if isize is not None:
        struct.pack_into("<I", b, 32, isize & 0xffffffff)
    return bytes(b)


def side(r):
    c = core(r)
    s = (b"1" if c["flag"] & 0x40 else b"2") + (b"R" if c["flag"] & 0x10 else b"F")
    for w in cigar(r):
        if w & 15 > 10:
            raise Undefined("a CIGAR op above 10 in a CT field")
        s += b"%d" % (w >> 4) + CIGAR_STR[w & 15:(w & 15) + 1]
    return s


def template_cigar(b1, b2):
    """bam_template_cigar -> (b1, b2) with the CT field behind the lower one, or as they are"""
    c1, c2 = core(b1), core(b2)
    if c1["tid"] != c2["tid"] or c1["tid"] < 0:
        return b1, b2, 0
    swap = c1["pos"] > c2["pos"]
    lo, hi = (b2, b1) if swap else (b1, b2)
    text = side(lo) + b"%d" % wrap(core(hi)["pos"] - calend(lo)) + b"T" + side(hi)
    grown = lo + b"CTZ" + text + b"\0"
    grown = struct.pack("<i", len(grown) - 4) + grown[4:]
    return (b1, grown, len(grown) - len(lo)) if swap else (grown, b2, len(grown) - len(lo))


def machine(recs, target_len, remove_reads):
    """bam_mating_core's loop -> ([(ordinal, record as written)], counts)"""
    out = []
    n = {"pairs": 0, "singletons": 0, "tags": 0, "added": 0}
    pre = None          # (ordinal, record, its end)
    for i, cur in enumerate(recs):
        c = core(cur)
        if c["tid"] < 0:
            if not remove_reads:
                out.append((i, cur))
            continue
        end = calend(cur)
        if c["tid"] >= len(target_len):
            raise Undefined("a refID the header does not have")
        if end > wrap(target_len[c["tid"]]):
            cur = with_core(cur, flag=c["flag"] | 0x4)
            c = core(cur)
        if c["flag"] & 0x100:
            if not remove_reads:
                out.append((i, cur))
            continue
        if pre is None:
            pre = (i, cur, end)
            continue
        j, p, pend = pre
        pc = core(p)
        if qname(cur) == qname(p):
            cf, pf = c["flag"], pc["flag"]
            if pc["tid"] == c["tid"] and not cf & 0xc and not pf & 0xc:
                cur5 = end if cf & 0x10 else c["pos"]
                pre5 = pend if pf & 0x10 else pc["pos"]
                ci, pi = pre5 - cur5, cur5 - pre5
            else:
                ci = pi = 0
            cf = cf | 0x20 if pf & 0x10 else cf & ~0x20
            pf = pf | 0x20 if cf & 0x10 else pf & ~0x20
            if cf & 0x4:
                pf = (pf | 0x8) & ~0x2
            if pf & 0x4:
                cf = (cf | 0x8) & ~0x2
            cur = with_core(cur, flag=cf, mtid=pc["tid"], mpos=pc["pos"], isize=ci)
            p = with_core(p, flag=pf, mtid=c["tid"], mpos=c["pos"], isize=pi)
            p, cur, added = template_cigar(p, cur)
            n["pairs"] += 1
            n["tags"] += 1 if added else 0
            n["added"] += added
            out += [(j, p), (i, cur)]
            pre = None
        else:
            pf = pc["flag"]
            if pf & 0x1:
                pf = (pf | 0x8) & ~0x20 & ~0x2
            out.append((j, with_core(p, flag=pf, mtid=-1, mpos=-1, isize=0)))
            n["singletons"] += 1
            pre = (i, cur, end)
    if pre is not None:
        out.append((pre[0], pre[1]))
    return out, n


def fixmate(data, remove_reads=False):
    """-> (the output file's bytes or None, stderr, status); status 2 where the reference's behaviour is undefined"""
    p = parse(data)
    if not p.ok:
        return None, None, 2
    err = p.err.replace("[bam_sort_core] truncated file. Continue anyway.\n", "")       # (bam_mating_core's loop ends without a word)
    try:
        out, _ = machine(p.recs, [ln for _, ln in p.targets], remove_reads)
    except Undefined:
        return None, None, 2
    blocks = cut(header_bytes(p.text, p.targets), [r for _, r in out])
    return b"".join(member(b, -1) for b in blocks) + EOF_BLOCK, err, 0


def classes(recs, target_len):
    """per record: LIVE, SKIP_TID or SKIP_SECONDARY -- from the flag behind the 0x4 update"""
    out = []
    for r in recs:
        c = core(r)
        if c["tid"] < 0:
            out.append(SKIP_TID)
        else:
            flag = c["flag"] | (0x4 if calend(r) > wrap(target_len[c["tid"]]) else 0)
            out.append(SKIP_SECONDARY if flag & 0x100 else LIVE)
    return out


def closed_form(cls, names, remove_reads):
    """The device's formulation.  cls: per record LIVE or not; names: per record its name (looked at for live records only).
    -> (roles, order): the role of every record, and the ordinals in the order the reference writes them."""
    n = len(cls)
    live = [i for i in range(n) if cls[i] == LIVE]
    head = [l == 0 or names[live[l]] != names[live[l - 1]] for l in range(len(live))]
    start, at = 0, []
    for l in range(len(live)):      # the place inside the run of equal names (on the device: two scans)
        if head[l]:
            start = l
        at.append(l - start)
    roles, writes = [SKIPPED] * n, [0 if remove_reads else 1] * n
    for l, i in enumerate(live):
        next_same = l + 1 < len(live) and not head[l + 1]
        roles[i] = SECOND if at[l] & 1 else FIRST if next_same else PENDING if l + 1 == len(live) else SINGLE
        writes[i] = (1 if l > 0 and not at[l - 1] & 1 else 0) + (at[l] & 1)
    woff = [0]
    for w in writes:
        woff.append(woff[-1] + w)
    order = [None] * (woff[n] + (1 if PENDING in roles else 0))
    ordinal = {i: l for l, i in enumerate(live)}
    for i in range(n):
        ro = roles[i]
        if ro == SKIPPED:
            if writes[i]:
                order[woff[i]] = i
        elif ro == PENDING:
            order[woff[n]] = i                                 # behind everything a record triggered
        elif ro in (SINGLE, FIRST):
            order[woff[live[ordinal[i] + 1]]] = i              # the next live record writes it first
        else:
            order[woff[i] + 1] = i
    return roles, order


def device_reason(recs, n_targets):
    """(ordinal, reason) of the first record outside the device's domain, or None (reasons: include/hpngs.h)"""
    for i, r in enumerate(recs):
        c = core(r)
        if c["tid"] < 0:
            continue
        if c["tid"] >= n_targets:
            return i, 3
        if len(r) < 36 or 36 + c["l_qname"] + 4 * c["n_cigar"] > len(r):
            return i, 4
        reason = 1 if any(w & 15 > 8 for w in cigar(r)) else 0
        if not reason and not c["flag"] & 0x100:
            nm = r[36:36 + c["l_qname"]]
            if not nm or nm.find(b"\0") != len(nm) - 1:
                reason = 2
        if reason:
            return i, reason
    return None


def route(data):
    """'device' where the record index takes the file and every record lies inside the device's domain; else 'host'"""
    if index_route(data) != "device":
        # (bam_sort's pos bound is its own; the index refuses only what lies below -1)
        p = parse(data)
        if not p.ok or p.err.count("truncated"):
            return "host"
        for r in p.recs:
            c = core(r)
            if c["pos"] < -1 or c["tid"] < -1 or c["mtid"] < -1 or c["mpos"] < -1:
                return "host"
    p = parse(data)
    return "host" if device_reason(p.recs, len(p.targets)) else "device"
