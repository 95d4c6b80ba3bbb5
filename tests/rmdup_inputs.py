"""Inputs of the recorded `samtools rmdup` runs (tests/golden/make_golden_rmdup.py) and of the tests that replay them: small
coordinate-sorted BAM files from fixed seeds, built here record by record and never stored -- the manifest holds their SHA-256.
Every file is named after what it is there for."""
import hashlib
import os
import struct

import numpy as np

from bai_inputs import FULL, bgzf, header, lay_packed, lay_sam, refs
from bamsort_inputs import noise

RG_LINES = "@RG\tID:a\tLB:libA\n@RG\tID:b\tLB:libB\tSM:s\n@RG\tID:a2\tSM:s\tLB:libA\n@RG\tID:nolb\tSM:s\n"
L = 20          # read length of the generated pairs


def text_with(rg=RG_LINES, n_ref=3, extra=""):
    return "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs(n_ref)) + rg + extra


H3 = header(refs(3), text_with())


def rec(tid, pos, name, flag, isize=0, qual=b"", mtid=None, mpos=0, aux=b"", cigar=(), raw_name=None):
    """one record; name: str or bytes without its NUL (raw_name: the l_read_name bytes as they are)"""
    nm = raw_name if raw_name is not None else (name.encode() if isinstance(name, str) else name) + b"\0"
    mtid = tid if mtid is None else mtid
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), 30, 4680, len(cigar), flag, len(qual), mtid, mpos, isize)
    body += nm + struct.pack("<%dI" % len(cigar), *cigar) + bytes((len(qual) + 1) // 2) + qual + aux
    return struct.pack("<i", len(body)) + body


def rg(ident):
    return b"" if ident is None else b"RGZ" + ident.encode() + b"\0"


def q(value, n=L):
    return bytes([value]) * n


def head(tid, pos, name, isize, qual, ident="a", aux=None, flag=0x63):
    return rec(tid, pos, name, flag, isize, qual, mpos=pos + isize - L, aux=rg(ident) if aux is None else aux, cigar=(len(qual) << 4,) if qual else ())


def tail(tid, pos, name, isize, ident="a", flag=0x93, qual=None):
    qual = q(30) if qual is None else qual
    return rec(tid, pos, name, flag, -isize, qual, mpos=pos - isize + L, aux=rg(ident), cigar=(len(qual) << 4,))


def single(tid, pos, name, flag=0, qual=None, ident="a", cig=None):
    qual = q(30) if qual is None else qual
    return rec(tid, pos, name, flag, 0, qual, mtid=-1, mpos=-1, aux=rg(ident), cigar=(len(qual) << 4,) if cig is None else cig)


def unplaced(name):
    return rec(-1, -1, name, 4, 0, q(20), mtid=-1, mpos=-1)


def in_order(items):
    """(tid, pos, record) in any order -> the records by (unsigned tid, pos), ties as given"""
    return [r for _, _, r in sorted(items, key=lambda t: (t[0] & 0xffffffff, t[1]))]


def pairs(frags, prefix="f"):
    """frags: (tid, pos, isize, RG ID, [quality values]) -> one pair per value: heads at pos, tails at pos + isize - L"""
    items = []
    for f, (tid, pos, isize, ident, quals) in enumerate(frags):
        for k, v in enumerate(quals):
            name = "%s%d_%d" % (prefix, f, k)
            qual = v if isinstance(v, bytes) else q(v)
            items.append((tid, pos, head(tid, pos, name, isize, qual, ident)))
            items.append((tid, pos + isize - L, tail(tid, pos + isize - L, name, isize, ident)))
    return items


def mixed(seed, n=120, unpl=5):
    """the general case: duplicated pairs of several libraries over three targets, single reads, mates elsewhere, unplaced"""
    rs = np.random.RandomState(seed)
    frags, items = [], []
    for f in range(n):
        tid, pos = int(rs.randint(0, 3)), int(rs.randint(0, 60)) * 50
        frags.append((tid, pos, int(rs.choice([100, 150, 151])), [None, "a", "b", "a2", "nolb", "zz"][int(rs.randint(0, 6))],
                      [int(v) for v in rs.randint(10, 14, int(rs.choice([1, 1, 2, 3, 5])))]))
    items += pairs(frags)
    for k in range(n // 3):
        tid, pos = int(rs.randint(0, 3)), int(rs.randint(0, 60)) * 50
        kind = int(rs.randint(0, 4))
        if kind == 0:
            items.append((tid, pos, single(tid, pos, "s%d" % k, 16 * int(rs.randint(0, 2)), q(int(rs.randint(10, 14))))))
        elif kind == 1:
            items.append((tid, pos, rec(tid, pos, "x%d" % k, 0x41, 500, q(30), mtid=(tid + 1) % 3, mpos=7)))          # the mate on another target
        elif kind == 2:
            items.append((tid, pos, rec(tid, pos, "m%d" % k, 0x49, 0, q(30), mpos=pos)))                             # the mate unmapped
        else:
            items.append((tid, pos, rec(tid, pos, "e%d" % k, 0x43, 120, q(30), mtid=-1, mpos=pos + 100, aux=rg("b"))))   # mtid -1: still a head
    return in_order(items) + [unplaced("u%d" % k) for k in range(unpl)]


def qual_lengths():
    """sum_qual over l_seq of 0 .. 300, quality bytes of 0xff among them: three heads a group, the winner in each place"""
    items = []
    for g, n in enumerate((0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300)):          # (300 x 0xff: a sum beyond 16 bits)
        for w in range(3):
            pos = 1000 * g + 100 * w
            for k in range(3):
                qual = (q(0xff, n) if k == w else q(0xfe, n - 1) + b"\xff") if n else b""
                items.append((0, pos, head(0, pos, "l%d_%d_%d" % (n, w, k), 300, qual)))
                items.append((0, pos + 300, tail(0, pos + 300, "l%d_%d_%d" % (n, w, k), 300)))
    return in_order(items)


def groups():
    """groups of 1, 2, 3, 64, 65 and 300 heads with sums rising, falling, all equal and with the winner last"""
    frags = []
    for g, n in enumerate((1, 2, 3, 64, 65, 300)):
        sums = lambda v: bytes([min(v, 250), v - min(v, 250)]) + q(1, L - 2)          # qualities that add up to v + L - 2
        shapes = {"rising": [sums(k) for k in range(n)], "falling": [sums(n - 1 - k) for k in range(n)], "equal": [17] * n, "last": [12] * (n - 1) + [13]}
        for s, (shape, quals) in enumerate(sorted(shapes.items())):
            frags.append((g % 2, 5000 * g + 500 * s, 200, "a", quals))
    return in_order(pairs(frags, "g"))


def interleaved():
    """four isize values and four libraries in turn at one pos, and the same again at the next"""
    items = []
    for pos in (700, 701):
        for k in range(48):
            isize, ident = (100, 101, 150, 4000)[k % 4], ("a", "b", "a2", None)[(k // 4) % 4]
            name = "i%d_%d" % (pos, k)
            items.append((1, pos, head(1, pos, name, isize, q(10 + (k * 7) % 5), ident)))
            items.append((1, pos + isize - L, tail(1, pos + isize - L, name, isize, ident)))
    return in_order(items)


def batches():
    """one group spread over ingest batches and BGZF blocks (records of ~750 bytes that do not compress); the tails far behind"""
    items = []
    for k in range(300):
        if k % 5 == 0:
            items.append((1, 777, rec(1, 777, "q%d" % k, 0x63, 250, q(10 + k % 9), mpos=1007, aux=rg("a") + noise(k, 700), cigar=(L << 4,))))
            items.append((1, 100000 + k, tail(1, 100000 + k, "q%d" % k, 250)))
        else:
            items.append((k % 3, 1000 + 37 * (k * 7919 % 300), rec(k % 3, 1000 + 37 * (k * 7919 % 300), "p%d" % k, 0, 0, q(30), mtid=-1, mpos=-1, aux=noise(k, 700))))
    return in_order(items)


def tails():
    t = []
    t += [tail(0, 100, "front", 50), head(0, 100, "front", 50, q(10)), head(0, 100, "front2", 50, q(9))]          # a tail in front of its head at one pos
    t += [head(0, 200, "d1", 80, q(10)), head(0, 200, "d2", 80, q(10)), tail(0, 260, "d1", 80), tail(0, 260, "d2", 80)]      # d2's tail is dropped
    t += [head(0, 300, "w1", 80, q(10)), head(0, 300, "w2", 80, q(11)), tail(0, 360, "w1", 80), tail(0, 360, "w1", 80), tail(0, 360, "w2", 80)]   # twice
    t += [head(0, 400, "n1", 80, q(10)), head(0, 400, "n2", 80, q(10)), head(0, 400, "n3", 80, q(12))]           # n1, n2: no mate before the target ends
    t += [head(1, 10, "n2", 80, q(10)), tail(1, 70, "n2", 80), tail(1, 70, "n1", 80)]                               # ... and their names are free again
    t += [head(2, 10, "z1", 80, q(10)), head(2, 10, "z2", 80, q(10)), head(2, 10, "z3", 80, q(10))]               # losers at the end of the file
    return t


def names():
    """pairs of names that differ only in their last byte, at lengths 1, 15, 16, 17 and 254: one of each pair is a duplicate"""
    items = []
    for g, n in enumerate((1, 15, 16, 17, 254)):
        a, b = "n" * (n - 1) + "A", "n" * (n - 1) + "B"
        pos = 1000 * g
        items += [(0, pos, head(0, pos, a, 90, q(11))), (0, pos, head(0, pos, b, 90, q(10))),
                  (0, pos + 70, tail(0, pos + 70, a, 90)), (0, pos + 70, tail(0, pos + 70, b, 90))]
    return in_order(items)


def aux_of_every_type():
    one = [b"XAAx", b"Xcc\x80", b"XCC\x80", b"Xss\1\2", b"XSS\1\2", b"Xii\1\2\3\4", b"XII\1\2\3\4", b"Xff\0\0\x80\x3f", b"XZZtext\0", b"XHH1AF0\0"]
    arr = [b"XBB" + t + struct.pack("<i", 3) + bytes(3 * n) for t, n in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4))]
    return one + arr + [b"XBBc" + struct.pack("<i", 0)]


def rg_places():
    """RG as the first and the last tag and behind every aux type; no RG, an unknown ID, an @RG without LB, two IDs of one library;
    a tag named RG inside another field's value does not count"""
    t, pos = [], 100
    front = aux_of_every_type()
    cases = [rg("a") + b"".join(front), b"".join(front) + rg("a")] + [f + rg("a") for f in front] + [b"XZZRGZb\0" + rg("a")]
    for k, aux in enumerate(cases):
        t += [head(0, pos, "p%d_0" % k, 100, q(10), aux=aux), head(0, pos, "p%d_1" % k, 100, q(10), aux=rg("b")), head(0, pos, "p%d_2" % k, 100, q(10), aux=aux)]
        pos += 10
    for k, ident in enumerate((None, "zz", "nolb", "a", "a2", "b", None, "a2", "zz")):
        t.append(head(1, 500, "v%d" % k, 100, q(10 + k % 2), ident))
    return t


def se_reverse():
    """-s: reverse-strand reads that end at one place with the later one winning, forward ones replaced in place, paired reads
    passed through (-S: taken in)"""
    t = []
    for k in range(6):
        t.append(single(0, 100 + k, "r%d" % k, 16, q(10 + k), cig=((L - k) << 4,)))            # all end at 120; each beats the one before
    t += [single(0, 300, "f0", 0, q(10)), single(0, 300, "f1", 0, q(12)), single(0, 300, "f2", 0, q(11)), single(0, 300, "fb", 0, q(12), "b")]
    t += [head(0, 300, "p0", 100, q(10)), head(0, 300, "p1", 100, q(10)), rec(0, 305, "um", 4, 0, q(30), mtid=-1, mpos=-1)]
    t += [single(1, 300, "g0", 0, q(10)), single(1, 300, "g1", 16, q(10)), single(1, 300, "g2", 16, q(9))]
    return t + [unplaced("u0"), unplaced("u1")]


def residues():
    """600 records whose sizes take every residue mod 16, a third of them duplicates that leave"""
    rs = np.random.RandomState(3)
    items = []
    for k in range(200):
        pos = int(rs.randint(0, 400)) * 10
        for d in range(int(rs.randint(1, 4))):
            name = "r%d_%d" % (k, d) + "x" * int(rs.randint(0, 16))
            items.append((0, pos, head(0, pos, name, 100, q(int(rs.randint(10, 13))), aux=rg("a") + b"XZZ" + b"y" * int(rs.randint(0, 16)) + b"\0")))
            items.append((0, pos + 80, tail(0, pos + 80, name, 100)))
    return in_order(items)


def own_inputs():
    """name -> the file's bytes"""
    f = {}
    m = mixed(21)
    f["mixed"] = bgzf(lay_sam(H3, m))
    f["probe"] = bgzf(lay_sam(H3, tails()[:16]))
    f["qual_lengths"] = bgzf(lay_sam(H3, qual_lengths()))
    f["groups"] = bgzf(lay_sam(H3, groups()))
    f["interleaved"] = bgzf(lay_sam(H3, interleaved()))
    f["batches"] = bgzf(lay_sam(H3, batches()))
    f["tails"] = bgzf(lay_sam(H3, tails()))
    f["names"] = bgzf(lay_sam(H3, names()))
    f["rg_places"] = bgzf(lay_sam(H3, rg_places()))
    f["no_rg_lines"] = bgzf(lay_sam(header(refs(3)), m))
    f["rg_dup_id"] = bgzf(lay_sam(header(refs(3), text_with(RG_LINES + "@RG\tID:a\tLB:libC\n")), m))
    f["hd_no_tab"] = bgzf(lay_sam(header(refs(3), text_with(extra="@CO\n")), m[:60]))                  # sam_header_parse2 gives up, at every head again
    # the host's side of the domain
    few = in_order(pairs([(0, 100, 100, "a", [10, 11, 10]), (1, 50, 100, "b", [10, 10])]))
    f["rg_type_i"] = bgzf(lay_sam(H3, [head(0, 100, "t0", 100, q(10), aux=b"RGi\1\0\0\0"), head(0, 100, "t1", 100, q(11), aux=b"RGia\0\0\0")] + few))
    # (__skip_tag gives `d` no size: its eight bytes are walked as fields -- here a Z string that swallows the RG behind it)
    f["aux_d"] = bgzf(lay_sam(H3, [head(0, 100, "d0", 100, q(10), aux=b"XDd" + b"abZcdefg" + rg("b")), head(0, 100, "d1", 100, q(11), aux=rg("b"))] + few))
    f["inconsistent"] = bgzf(lay_sam(H3, [head(0, 100, "same", 100, q(11)), head(0, 100, "same", 100, q(10)), head(0, 100, "same", 100, q(10)),
                                          tail(0, 180, "same", 100), tail(0, 180, "same", 100)] + few[3:]))
    f["first_unplaced"] = bgzf(lay_sam(H3, [unplaced("u0"), rec(-1, 5, "u1", 0x43, 100, q(10), mpos=85), rec(-1, 5, "u2", 0x43, 100, q(11), mpos=85)] + few + [unplaced("u3")]))
    f["only_unplaced"] = bgzf(lay_sam(H3, [unplaced("u%d" % k) for k in range(5)]))
    f["no_records"] = bgzf([H3])
    f["tid_returns"] = bgzf(lay_sam(H3, in_order(pairs([(0, 100, 100, "a", [10, 11])])) + in_order(pairs([(1, 100, 100, "a", [10, 11])], "g")) +
                                    in_order(pairs([(0, 50, 100, "a", [10, 11])], "h"))))
    f["pos_m1"] = bgzf(lay_sam(H3, [head(0, -1, "m0", 100, q(10)), head(0, -1, "m1", 100, q(11)), rec(0, -1, "m2", 0, 0, q(10), mtid=-1, mpos=-1)] + few))
    # the writer
    f["residues"] = bgzf(lay_sam(H3, residues()))
    big = [head(0, 10, "full", 100, q(10), aux=rg("a") + b"XZZ" + b"a" * (FULL - len(head(0, 10, "full", 100, q(10), aux=rg("a") + b"XZZ\0"))) + b"\0"),
           head(0, 10, "over", 100, q(11), aux=rg("a") + b"XZZ" + b"a" * FULL + b"\0"), head(0, 10, "third", 100, q(10)),
           single(1, 5, "big", 0, q(30)), rec(1, 6, "huge", 0, 0, q(30), mtid=-1, mpos=-1, aux=b"XZZ" + b"b" * 70000 + b"\0")]
    assert len(big[0]) == FULL
    f["oversize"] = bgzf(lay_sam(H3, big[:3] + few[3:6] + big[3:] + few[6:]))
    f["hd_long"] = bgzf(lay_sam(header(refs(3), text_with(extra="".join("@CO\tline %d of a header longer than one block\n" % k for k in range(1700)))), m[:80]))
    f["packed_97"] = bgzf(lay_packed(H3, m[:150], 97))
    f["packed_1000"] = bgzf(lay_packed(H3, m, 1000))
    f["no_eof"] = bgzf(lay_sam(H3, m[:80]), eof=False)
    whole = bgzf(lay_sam(H3, m))
    f["trunc_bytes"] = whole[:len(whole) * 2 // 3]
    f["se_reverse"] = bgzf(lay_sam(H3, se_reverse()))
    return f


def unsorted_stale():
    """NOT a recorded case (the reference reads freed memory): pos 100, 200, and 100 again with the key of a group already written"""
    return bgzf(lay_sam(H3, [head(0, 100, "a", 100, q(10)), head(0, 200, "b", 100, q(10)), head(0, 100, "c", 100, q(10))]))


def tid_beyond():
    """NOT a recorded case: refID 7 of 3 -- the reference prints whatever lies behind its name table"""
    return bgzf(lay_sam(H3, [head(0, 100, "a", 100, q(10)), head(7, 100, "b", 100, q(10))]))


def materialize(directory):
    """writes every input as NAME.bam under `directory`; returns {file name: sha256}"""
    digests = {}
    for name, data in own_inputs().items():
        with open(os.path.join(directory, name + ".bam"), "wb") as fh:
            fh.write(data)
        digests[name + ".bam"] = hashlib.sha256(data).hexdigest()
    return digests


def names_of_inputs():
    return sorted(own_inputs())


def path_of(name, made):
    return os.path.join(made, name + ".bam")
