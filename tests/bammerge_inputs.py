"""Inputs of the recorded `samtools merge` runs (tests/golden/make_golden_bammerge.py) and of the tests that replay them: SETS of
small BAM files from fixed seeds -- a set is the list of one run's inputs in argument order --, built with the helpers of
tests/bai_inputs.py and never stored: the manifest holds their SHA-256.  Every set is named after what it is there for.  In a
run's directory the files of a set are in1.bam, in2.bam, ...; header files for -h are text (header_files())."""
import hashlib
import os
import struct

import numpy as np

import bam_layouts
from bai_inputs import FULL, bgzf, header, lay_sam, mixed, rec, refs
from bamsort_inputs import moved, noise, shuffled, sized, text_with

HD = "@HD\tVN:1.0\tSO:coordinate\n"


def key(r):
    """the heap's key of an encoded record"""
    tid, pos, _, flag_nc = struct.unpack_from("<iiII", r, 4)
    return ((tid << 32) & (1 << 64) - 1) | (((pos + 1) << 1) & 0xffffffff) | (flag_nc >> 20 & 1)


def by_key(recs):
    return sorted(recs, key=key)


def deal(recs, n, seed):
    """the records dealt to n files at random, every file then in key order"""
    rs = np.random.RandomState(seed)
    to = rs.randint(0, n, len(recs))
    return [by_key([r for r, t in zip(recs, to) if t == k]) for k in range(n)]


def bam(recs, hdr=None):
    return bgzf(lay_sam(hdr if hdr is not None else header(refs(3)), recs))


def own_sets():
    """name -> the set's files (bytes), in argument order"""
    s = {}
    h3 = header(refs(3))
    base = mixed(21, per=40, unplaced=6)
    s["two_sorted"] = [bam(f) for f in deal(base, 2, 1)]
    s["three_sorted"] = [bam(f) for f in deal(mixed(22, per=60, unplaced=9), 3, 2)]
    # one key in every file, and both strands at one position in every file
    eq = lambda f: [rec(1, 500, "20M", 0, "e%d_%d" % (f, k), pad=5 + (f + k) % 7) for k in range(5)]
    s["equal_keys"] = [bam(by_key(eq(f) + [rec(0, 10 + f, "10M", 0, "a%d" % f), rec(2, 90 - f, "10M", 0, "z%d" % f)])) for f in range(3)]
    st = lambda f: [rec(1, 5000, "30M", 16 * (k & 1), "s%d_%d" % (f, k)) for k in range(8)]
    s["both_strands"] = [bam(by_key(st(f))) for f in range(3)]
    parts = deal(base, 2, 3)
    s["empty_first"] = [bam([]), bam(parts[0]), bam(parts[1])]
    s["empty_middle"] = [bam(parts[0]), bam([]), bam(parts[1])]
    s["empty_last"] = [bam(parts[0]), bam(parts[1]), bam([])]
    s["all_empty"] = [bam([]), bam([])]
    s["one_record"] = [bam(parts[0]), bam([rec(1, 100, "50M", 0, "only")])]
    up = [moved(rec(-1, 0, "", 4, "up%d" % k), p) for k, p in enumerate([5, 0, 700000, 5, -1, 3, 1 << 20])]
    s["unplaced_pos"] = [bam(f) for f in deal(base + up, 2, 4)]
    m1 = [rec(t, -1, "", 4 + 16 * (k & 1), "m%d" % k) for k, t in enumerate([0, 2, 1, 0, 2])]
    s["placed_pos_m1"] = [bam(f) for f in deal(base + m1, 2, 5)]
    # pos values the heap's key takes and bam1_lt's does not: forward strand, and reverse where the key is not HEAP_EMPTY
    hw = header(refs(3, (1 << 31) - 1))
    wide = [moved(rec(t, 0, "10M", f, "w%d" % k), p) for k, (t, p, f) in enumerate(
        [(1, (1 << 30) - 1, 0), (1, (1 << 31) - 1, 0), (1, -2, 0), (0, (1 << 30) - 1, 16), (0, (1 << 31) - 1, 16), (2, -2, 16),
         (-1, -2, 0), (-1, (1 << 31) - 2, 0), (-1, (1 << 31) - 1, 16), (-1, (1 << 30) - 1, 16)])]
    s["pos_wide"] = [bam(f, hw) for f in deal(base + wide, 2, 6)]
    s["pos_high"] = [bam(f, hw) for f in deal(base + [w for w in wide if struct.unpack_from("<i", w, 8)[0] >= 0], 2, 6)]      # (no pos below -1: the record index takes these)
    # HEAP_EMPTY: refID -1, reverse strand, pos -2 / 2^31 - 2 -- the largest key there is, so the file stays sorted with it last
    for name, pos in (("heap_empty_m2", -2), ("heap_empty_2p31m2", (1 << 31) - 2)):
        he = moved(rec(-1, 0, "", 4 + 16, "he"), pos)
        a, b = deal(base, 2, 7)
        s[name] = [bam(a + [he, he], hw), bam(b, hw)]
    s["heap_empty_mid"] = [bam(parts[0], hw), bam(parts[1][:10] + [moved(rec(-1, 0, "", 20, "he"), -2)] + parts[1][10:], hw)]
    # unsorted inputs: the reference merges them as they are
    big_first = by_key(parts[0])
    s["unsorted_first_largest"] = [bam([big_first[-1]] + big_first[:-1]), bam(parts[1])]
    s["unsorted_descending"] = [bam(by_key(parts[0])[::-1]), bam(parts[1])]
    mid = by_key([r for r in parts[0] if key(r) >> 32 != 0xffffffff])
    s["unsorted_unmapped_mid"] = [bam(mid[:20] + [rec(-1, -1, "", 4, "u_mid")] + mid[20:]), bam(parts[1])]
    s["unsorted_all"] = [bam(shuffled(f, 30 + k)) for k, f in enumerate(deal(mixed(23, per=50, unplaced=5), 3, 8))]
    # headers
    five = [rec(4, 7, "10M", 0, "far"), rec(3, 9, "10M", 0, "near")]
    s["more_targets_later"] = [bam(parts[0]), bam(by_key(parts[1] + five), header(refs(5))), bam([], header(refs(4)))]
    s["fewer_targets_later"] = [bam(by_key(parts[1] + five), header(refs(5))), bam(parts[0])]
    s["name_mismatch"] = [bam(parts[0]), bam(parts[1], header([("c0", 1 << 20), ("other", 1 << 20), ("c2", 1 << 20)]))]
    s["name_mismatch_beyond"] = [bam(parts[0], header(refs(2))), bam(parts[1], header([("c0", 1 << 20), ("c1", 1 << 20), ("x", 5)]))]
    s["hd_none"] = [bam(parts[0], header(refs(3), text_with(""))), bam(parts[1])]
    s["hd_second_differs"] = [bam(parts[0]), bam(parts[1], header(refs(3), text_with("@HD\tVN:1.4\tSO:unsorted\n") + "@CO\tsecond\n"))]
    s["hd_empty_text"] = [bam(parts[0], header(refs(3), "")), bam(parts[1])]
    long_text = text_with(HD) + "".join("@CO\tline %d of a header longer than one block\n" % k for k in range(1700))
    s["hd_long"] = [bam(parts[0], header(refs(3), long_text)), bam(parts[1])]
    # layouts and sizes
    rs = np.random.RandomState(0)
    res = [rec(int(rs.randint(0, 3)), int(rs.randint(0, 100000)), "10M", 16 * int(rs.randint(0, 2)), "n%d" % k, pad=5 + int(rs.randint(0, 48)))
           for k in range(1500)]
    s["residues"] = [bam(f) for f in deal(res, 3, 9)]
    over = [sized(0, 900, FULL, "full"), sized(0, 800, FULL + 1, "over"), sized(1, 5, 70000, "big")]
    s["oversize"] = [bam(f) for f in deal(base + over, 2, 10)]
    a, c = rec(0, 10, "10M", 0, "first"), rec(0, 30, "10M", 0, "third")
    s["exact_fill"] = [bam([a, c]), bam([sized(0, 20, FULL - len(a), "fills")])]
    s["packed"] = [bam_layouts.bgzf_pack(h3 + b"".join(f), n, eof=True) for f, n in zip(deal(res[:900], 3, 11), (97, 1000, 20000))]
    s["no_eof"] = [bam(parts[0]), bgzf(lay_sam(h3, parts[1]), eof=False)]
    nz = [rec(k % 3, 1000 + 37 * (k * 7919 % 300), "20M", 0, "p%d" % k, aux=noise(k, 700)) for k in range(300)]
    s["incompressible"] = [bam(f) for f in deal(nz, 2, 12)]
    s["seventeen"] = [bam(f) for f in deal(mixed(24, per=80, unplaced=12), 17, 13)]
    # -r: records with an RG of their own, in front of, between and behind other fields
    rg = []
    for k in range(40):
        aux = [b"NMC" + bytes([k]), b"RGZ" + b"lane%d\0" % (k % 3), b"XSA+", b"XBBS" + struct.pack("<iHH", 2, k, 7), b"ASi" + struct.pack("<i", -k)]
        aux = aux[k % 5:] + aux[:k % 5] if k % 2 else [x for x in aux if not x.startswith(b"RG")]
        rg.append(rec(k % 3, 50 * k, "10M", 0, "g%d" % k, aux=b"".join(aux)))
    s["rg_tagged"] = [bam(f) for f in deal(rg, 2, 14)]
    names = [rec(0, 10 * k, "10M", (0x40, 0x80, 0)[k % 3], "q%d" % (k // 3)) for k in range(60)]
    s["names"] = [bam(sorted(f, key=lambda r: (int(r[37:].split(b"\0")[0]), r[18] & 0xc0))) for f in deal(names, 3, 15)]
    return s


def header_files():
    """name -> the text of a -h file"""
    return {"h_match": text_with("@HD\tVN:1.4\tSO:coordinate\n") + "@RG\tID:x\tSM:y\n@CO\tfrom the header file\n",
            "h_no_sq": "@HD\tVN:1.4\tSO:coordinate\n@CO\tno sequence lines\n",
            "h_count": text_with(HD, 4),
            "h_name": HD + "@SQ\tSN:c0\tLN:1048576\n@SQ\tSN:cX\tLN:1048576\n@SQ\tSN:c2\tLN:1048576\n",
            "h_then_records": text_with(HD) + "r1\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n@CO\tnot a header line any more\n"}


def digests():
    """{set name: [sha256 of every file]}"""
    return {name: [hashlib.sha256(f).hexdigest() for f in files] for name, files in own_sets().items()}


def materialize(directory, name, files):
    """writes the set's files as in1.bam ... under `directory`; returns their names"""
    out = []
    for k, data in enumerate(files):
        fn = "in%d.bam" % (k + 1)
        with open(os.path.join(directory, fn), "wb") as fh:
            fh.write(data)
        out.append(fn)
    return out


def names():
    return sorted(own_sets())
