"""Inputs of the recorded `samtools view` runs (tests/golden/make_golden_view.py) and of the tests that replay them: small BAM files
from fixed seeds, never stored -- the manifest holds their SHA-256.  Every input is named after what it holds."""
import hashlib
import os
import struct

import numpy as np

from bai_inputs import FULL, bgzf, header, lay_sam, refs
from fixmate_inputs import words

SCAN_TILE = 2048      # docs/kernels/scan_sort.md: the scan's tile
NT16 = "=ACMGRSVTWYHKDBN"
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)


def rec(name, tid=-1, pos=-1, cigar="", flag=0, mapq=30, seq="", qual=None, mtid=-1, mpos=-1, isize=0, aux=b"", bin=4680):
    """one encoded record.  name: str or bytes (a NUL is added behind either); seq: letters of NT16 or a list of 4-bit codes; qual:
    None (absent: 0xff), or a list / bytes of l_seq values"""
    nm = (name.encode() if isinstance(name, str) else name) + b"\0"
    cg = words(cigar)
    codes = [NT16.index(c) for c in seq] if isinstance(seq, str) else list(seq)
    n = len(codes)
    packed = bytes((codes[i] << 4) | (codes[i + 1] if i + 1 < n else 0) for i in range(0, n, 2))
    ql = b"\xff" * n if qual is None else bytes(qual)
    assert len(ql) == n and len(nm) <= 255
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, bin, len(cg), flag, n, mtid, mpos, isize)
    body += nm + struct.pack("<%dI" % len(cg), *cg) + packed + ql + aux
    return struct.pack("<i", len(body)) + body


def read(rs, k, name=None, n=None, flag=None, aux=b"", tid=None, mapq=None):
    """a record as an aligner writes it"""
    n = int(rs.randint(20, 160)) if n is None else n
    tid = int(rs.randint(0, 3)) if tid is None else tid
    pos = int(rs.randint(0, 900000))
    paired = rs.randint(0, 4) != 0
    fl = (int(rs.choice([0x63, 0x93, 0x53, 0xa3, 0x41, 0x81, 0x49, 0x85])) if paired else int(rs.choice([0, 0x10, 0x4]))) if flag is None else flag
    if rs.randint(0, 10) == 0 and flag is None:
        fl |= 0x400
    cg = "%dM" % n if rs.randint(0, 3) else "%dS%dM%dI%dM" % (2, max(n - 12, 1), 3, 7) if n > 13 else "%dM" % n
    return rec(name or "r%d" % k, tid, pos, cg, fl, int(rs.randint(0, 61)) if mapq is None else mapq, [int(c) for c in rs.choice([1, 2, 4, 8, 15], n)],
               rs.randint(2, 42, n).tolist(), tid if paired else -1, pos + 200 if paired else -1, 350 if paired else 0, aux)


def bam(recs, hdr=None):
    return bgzf(lay_sam(hdr if hdr is not None else header(refs(3)), recs))


def aux_i(key, typ, v):
    return key + typ.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ], v)


def aux_b(key, sub, vals):
    return key + b"B" + sub.encode() + struct.pack("<i", len(vals)) + b"".join(struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[sub], v)
                                                                               for v in vals)


RG_TEXT = ("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs(3)) +
           "@RG\tID:a1\tLB:libA\tSM:s\n@RG\tID:a2\tLB:libA\tSM:s\n@RG\tID:b1\tLB:libB\tSM:s\n@RG\tID:nolb\tSM:s\n@RG\tID:a1\tLB:libB\tSM:s\n@CO\tthe end\n")


def fill_block(rs, room, k0, flag=0):
    """records that take exactly `room` bytes: fillers of one size and one last record padded to fit"""
    mk = lambda k, pad: rec("f%05d" % k, 0, 10 + k, "50M", flag, 30, "A" * 50, rs.randint(40, 60, 50).tolist(), aux=b"XZZ" + b"p" * pad + b"\0")
    one = len(mk(0, 300))
    out, k = [], k0
    while room >= 2 * one:
        out.append(mk(k, 300))
        room -= one
        k += 1
    out.append(mk(k, 300 + room - one))
    assert len(out[-1]) == room
    return out


def cuts_input(delta):
    """kept records (flag 0) that fill the writer's first block exactly (delta 0), by one byte less or one more, dropped records
    (flag 0x400) between them, a kept record longer than a block whose quality bytes straddle the writer's cut, and a tail; qualities of 40..59 double past 93 under -Q 2"""
    rs = np.random.RandomState(31 + delta)
    hdr = header(refs(3))
    kept = fill_block(rs, FULL + delta, 0)
    out = []
    for k, r in enumerate(kept):
        out.append(r)
        if k % 7 == 3:
            out.append(rec("d%05d" % k, 1, 5, "10M", 0x400, seq="ACGTACGTAC", qual=[50] * 10))
    # longer than a block, and the block's end lies inside its quality bytes
    out.append(rec("long", 2, 77, "44000M", 0, seq="C" * 44000, qual=rs.randint(40, 60, 44000).tolist(), aux=b"XZZ" + b"q" * 100 + b"\0"))
    out += fill_block(rs, 3000, 9000) + [rec("d_end", 1, 5, "10M", 0x400, seq="ACGTACGTAC", qual=[50] * 10)]
    return bam(out, hdr)


def own_inputs():
    """name -> the file's bytes"""
    f = {}
    rs = np.random.RandomState(2026)
    # ---- lengths: l_qseq around the team's 16 lanes and the byte's two nibbles, qualities present and absent, name lengths
    ln = []
    for k, n in enumerate([0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257]):
        codes = [(i + k) % 16 for i in range(n)]
        ln.append(rec("len%d" % n, k % 3, 100 + k, "%dM" % n if n else "", 0x10 if k % 2 else 0, 20 + k, codes, [(i * 7 + k) % 94 for i in range(n)]))
        ln.append(rec("abs%d" % n, k % 3, 200 + k, "%dM" % n if n else "", 0, 20 + k, codes, None))
    for n in (1, 15, 16, 17, 254):
        ln.append(rec(("n" * n), 0, 5, "4M", 0, 7, "ACGT", [0, 1, 92, 93]))
    ln.append(rec("q0", 0, 5, "3M", 0, 7, "NNN", [0xff, 10, 20]))      # only the first quality byte says `absent`
    f["lengths"] = bam(ln)
    # ---- numbers: every integer field at its digit boundaries and ends
    nu = []
    edges = [-1, 0, 8, 9, 98, 99, 998, 999, 9998, 9999, 99998, 99999, 999998, 999999, 9999998, 9999999, 99999998, 99999999, 999999998, 999999999, I32_MAX - 1]
    wide = header(refs(3, I32_MAX))
    for k, p in enumerate(edges):
        nu.append(rec("pos%d" % k, 0, p, "5M", 0, 30, "ACGTA", [30] * 5, 1, edges[-1 - k], 0))
    for k, v in enumerate([I32_MIN, -1, 0, I32_MAX, -9, -10, 9, 10, -99999, 100000]):
        nu.append(rec("isize%d" % k, 1, 50, "5M", 0x1, 30, "ACGTA", [30] * 5, 1, 60, v))
    for k, q in enumerate([0, 9, 10, 99, 100, 255]):
        nu.append(rec("mapq%d" % q, 2, 50, "5M", 0, q, "ACGTA", [30] * 5))
    for fl in [0, 0xffff, 0xf, 0x10, 0xff, 0x100, 0xfff, 0x1000] + [1 << b for b in range(16)]:
        nu.append(rec("flag%x" % fl, 0, 50, "5M", fl, 30, "ACGTA", [30] * 5))
    big = (1 << 28) - 1
    nu.append(rec("ops", 0, 50, [(k + 1, k) for k in range(10)], 0, 30, "ACGTA", [30] * 5))
    nu.append(rec("oplen", 0, 50, [(0, 0), (big, 0), (big, 3), (9, 1), (10, 1), (99, 4), (100, 5)], 0, 30, "ACGTA", [30] * 5))
    nu.append(rec("nocigar", 0, 50, "", 0, 30, "ACGTA", [30] * 5))
    nu.append(rec("manyops", 1, 50, [(1 + k % 120, (0, 1, 0, 2, 4, 5)[k % 6]) for k in range(65535)], 0, 30, "ACGTA", [30] * 5))
    f["numbers"] = bam(nu, wide)
    # ---- aux_all: every type at its extremes, arrays, strings; no floats
    au = []
    ints = b"".join([aux_i(b"c0", "c", -128), aux_i(b"c1", "c", 127), aux_i(b"c2", "c", 0), aux_i(b"C0", "C", 0), aux_i(b"C1", "C", 255), aux_i(b"s0", "s", -32768),
                     aux_i(b"s1", "s", 32767), aux_i(b"S0", "S", 0), aux_i(b"S1", "S", 65535), aux_i(b"i0", "i", I32_MIN), aux_i(b"i1", "i", I32_MAX),
                     aux_i(b"i2", "i", -1), aux_i(b"I0", "I", 0), aux_i(b"I1", "I", 0xffffffff), aux_i(b"I2", "I", 1 << 31)])
    au.append(rec("ints", 0, 10, "4M", 0, 30, "ACGT", [30] * 4, aux=ints))
    au.append(rec("chars", 0, 11, "4M", 0, 30, "ACGT", [30] * 4, aux=b"XAA!XBA~XCA\tXDA\xff"))
    au.append(rec("strings", 0, 12, "4M", 0, 30, "ACGT", [30] * 4, aux=b"Z0Z\0Z1Zx\0Z2Zhello world\0H0H\0H1H1AE301\0Z3Z\xe9\x80\0"))
    arrays = b"".join([aux_b(b"Bc", "c", [-128, 0, 127]), aux_b(b"BC", "C", [0, 9, 10, 255]), aux_b(b"Bs", "s", [-32768, 32767]), aux_b(b"BS", "S", [0, 65535, 100]),
                       aux_b(b"Bi", "i", [I32_MIN, I32_MAX, -1, 0]), aux_b(b"BI", "I", [0, 0xffffffff]), aux_b(b"Be", "c", []), aux_b(b"BE", "I", [])])
    au.append(rec("arrays", 1, 13, "4M", 0, 30, "ACGT", [30] * 4, aux=arrays))
    au.append(rec("longz", 1, 14, "4M", 0, 30, "ACGT", [30] * 4, aux=b"LZZ" + bytes(33 + (i * 11) % 90 for i in range(60000)) + b"\0" + aux_i(b"NM", "C", 3)))
    au.append(rec("many", 2, 15, "4M", 0, 30, "ACGT", [30] * 4, aux=b"".join(aux_i(b"%c%c" % (65 + k % 26, 97 + k // 26), "CcSsIi"[k % 6], k % 100) for k in range(300))))
    au.append(rec("longarray", 2, 16, "4M", 0, 30, "ACGT", [30] * 4, aux=aux_b(b"BL", "s", [((i * 7919) % 65536) - 32768 for i in range(5000)])))
    au.append(rec("noseq_aux", 2, 17, "", 0, 30, "", None, aux=aux_i(b"NM", "i", 5) + b"RGZgrp\0"))
    f["aux_all"] = bam(au)
    # ---- the host-route inputs
    floats = [0.0, 1.0, -1.5, 100000.0, 1000000.0, 123456.0, 1234567.0, 0.0001, 0.00001, 3.14159274, 1e38, -1e-38, float("inf"), float("-inf"), float("nan"), 0.1]
    fl = [rec("f%d" % k, 0, 10 + k, "4M", 0, 30, "ACGT", [30] * 4, aux=b"XFf" + struct.pack("<f", v) + aux_i(b"NM", "C", k)) for k, v in enumerate(floats)]
    fl.append(rec("dbl", 0, 50, "4M", 0, 30, "ACGT", [30] * 4, aux=b"XDd" + struct.pack("<d", 2.5e-300) + b"YDd" + struct.pack("<d", 123456789.125)))
    fl.append(rec("bf", 0, 51, "4M", 0, 30, "ACGT", [30] * 4, aux=aux_b(b"BF", "f", floats[:12]) + aux_b(b"Bf", "f", [])))
    f["aux_float"] = bam([read(rs, k) for k in range(20)] + fl)
    f["aux_a_nul"] = bam([read(rs, k) for k in range(5)] + [rec("anul", 0, 10, "4M", 0, 30, "ACGT", [30] * 4, aux=b"XAA\0" + aux_i(b"NM", "C", 1)), read(rs, 6)])
    f["name_nul_inside"] = bam([read(rs, 0), rec(b"ab\0x", 0, 10, "4M", 0, 30, "ACGT", [30] * 4), rec(b"ab\0y", 0, 50, "4M", 0x10, 30, "ACGT", [30] * 4), read(rs, 3)])
    f["aux_unknown"] = bam([read(rs, 0), rec("unk", 0, 10, "4M", 0, 30, "ACGT", [30] * 4, aux=b"XQq" + aux_i(b"NM", "C", 1)), read(rs, 2)])
    f["aux_b_negative"] = bam([read(rs, 0), rec("bneg", 0, 10, "4M", 0, 30, "ACGT", [30] * 4, aux=b"XBBc" + struct.pack("<i", -3) + aux_i(b"NM", "C", 1)), read(rs, 2)])
    # ---- rg: two libraries over three IDs, an @RG without LB, a duplicated ID; RG of type Z and of another type, none, an unknown ID
    rg = []
    tags = [b"RGZa1\0", b"RGZa2\0", b"RGZb1\0", b"RGZnolb\0", b"RGZzz\0", b"", aux_i(b"RG", "C", 65) + aux_i(b"NM", "C", 0), b"XYZRG\0RGZb1\0", aux_i(b"NM", "C", 2) + b"RGZa1\0"]
    for k in range(90):
        rg.append(read(rs, k, aux=tags[k % len(tags)]))
    f["rg"] = bam(rg, header(refs(3), RG_TEXT))
    f["rg_clean"] = bam(rg, header(refs(3), RG_TEXT.replace("@RG\tID:a1\tLB:libB\tSM:s\n", "")))       # no ID twice: the table is made without a word
    # ---- subsample: names with bytes >= 0x80, of one byte, pairs sharing a name
    ss = []
    for k in range(300):
        nm = b"t%d" % k if k % 3 else bytes([0x80 + k % 128, 0xc3, 0x28 + k % 80, 0xff])
        ss += [read(rs, k, name=nm, flag=0x63), read(rs, k, name=nm, flag=0x93)]
    ss += [read(rs, k, name=bytes([c])) for k, c in enumerate([1, 0x41, 0x7f, 0x80, 0xff])]
    f["subsample"] = bam(ss)
    # ---- runs: kept (flag 0) and dropped (flag 0x400) runs around the scan's tile
    small = lambda k, fl: rec("u%d" % k, k % 3, k, "3M", fl, 30, "ACG", [30 + k % 10] * 3)
    ru, k = [], 0
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        for fl in (0, 0x400):
            ru += [small(k + j, fl) for j in range(n)]
            k += n
    f["runs"] = bam(ru)
    f["last_only"] = bam([small(j, 0x400) for j in range(SCAN_TILE + 100)] + [small(9, 0)])
    f["no_records"] = bam([])
    # ---- cuts
    f["cuts_exact"], f["cuts_less"], f["cuts_more"] = cuts_input(0), cuts_input(-1), cuts_input(1)
    # ---- mixed
    mx = []
    for k in range(3000):
        aux = b"".join([aux_i(b"NM", "C", k % 7), b"MDZ%d\0" % (k % 150), aux_i(b"AS", "i", -k), aux_b(b"XB", "S", [k % 9, k % 11]) if k % 5 == 0 else b""])
        mx.append(read(rs, k, aux=aux) if k % 97 else rec("un%d" % k, -1, -1, "", 0x4, 0, "ACGTN" * 8, None))
    f["mixed"] = bam(mx)
    # ---- the text header
    f["hdr_no_sq"] = bam([read(rs, k) for k in range(4)], header(refs(3), ""))
    f["hdr_mismatch"] = bam([read(rs, k) for k in range(4)], header(refs(3), "@HD\tVN:1.0\n@SQ\tSN:c0\tLN:5\n@CO\tone line for three targets\n"))
    # ---- damaged files
    whole = f["mixed"]
    f["truncated_mid_block"] = whole[:len(whole) // 2]
    pieces = lay_sam(header(refs(3)), mx[:600])
    f["truncated_mid_record"] = bgzf(pieces[:-1] + [pieces[-1][:len(pieces[-1]) - 37]])
    f["no_eof"] = bgzf(lay_sam(header(refs(3)), mx[:50]), eof=False)
    # ---- refused
    f["tid_beyond_header"] = bam([read(rs, 0), rec("far", 3, 10, "4M", 0, 30, "ACGT", [30] * 4)])
    f["mtid_beyond_header"] = bam([read(rs, 0), rec("farmate", 1, 10, "4M", 0x1, 30, "ACGT", [30] * 4, 7, 10, 0)])
    return f


_CACHE = {}


def inputs():
    if not _CACHE:
        _CACHE.update(own_inputs())
    return _CACHE


def digests():
    return {name: hashlib.sha256(data).hexdigest() for name, data in inputs().items()}


def materialize(directory, name, data):
    with open(os.path.join(directory, "in.bam"), "wb") as fh:
        fh.write(data)
    return "in.bam"


def names():
    return sorted(inputs())
