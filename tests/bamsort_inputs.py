"""Inputs of the recorded `samtools sort` runs (tests/golden/make_golden_bamsort.py) and of the tests that replay them: small BAM
files from fixed seeds, built with the helpers of tests/bai_inputs.py and never stored -- the manifest holds their SHA-256.
Every file is named after what it is there for."""
import hashlib
import os
import struct

import numpy as np

from bai_inputs import FULL, bgzf, header, lay_packed, lay_sam, mixed, rec, refs

HD_SORTED = "@HD\tVN:1.0\tSO:coordinate\n"


def shuffled(recs, seed):
    rs = np.random.RandomState(seed)
    return [recs[i] for i in rs.permutation(len(recs))]


def noise(seed, n):
    """an aux field of n incompressible bytes (a `B` array of uint8)"""
    return b"XBBC" + struct.pack("<i", n) + np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def moved(r, pos):
    """the record with another pos (the helpers derive the bin from it, which only exists below 2^29)"""
    b = bytearray(r)
    struct.pack_into("<i", b, 8, pos if pos < 1 << 31 else pos - (1 << 32))
    return bytes(b)


def sized(tid, pos, size, name="z", flag=0):
    """a record of exactly `size` bytes"""
    base = len(rec(tid, pos, "10M", flag, name))
    assert size - base >= 5
    r = rec(tid, pos, "10M", flag, name, pad=size - base)
    assert len(r) == size
    return r


def text_with(hd, n_ref=3):
    return hd + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs(n_ref))


def strands():
    """the general case: placed records of three targets, unplaced ones, and 200 records of one (refID, pos) on both strands"""
    same = [rec(1, 5000, "30M", 16 * (k & 1), "s%d" % k) for k in range(200)]
    return shuffled(mixed(13, per=100, unplaced=10) + same, 5)


def residues():
    """1,000 records whose sizes take every residue mod 16; the seed is one for which every (source, destination) pair of residues
    occurs after sorting (256 pairs: fewer records leave some out)"""
    rs = np.random.RandomState(0)
    return [rec(int(rs.randint(0, 3)), int(rs.randint(0, 100000)), "10M", 16 * int(rs.randint(0, 2)), "n%d" % k, pad=5 + int(rs.randint(0, 48)))
            for k in range(1000)]


def own_inputs():
    """name -> the file's bytes"""
    f = {}
    h3 = header(refs(3))
    base = mixed(11)
    f["no_records"] = bgzf([h3])
    f["one_record"] = bgzf(lay_sam(h3, [rec(1, 100, "50M")]))
    f["sorted"] = bgzf(lay_sam(h3, base))
    f["reversed"] = bgzf(lay_sam(h3, base[::-1]))
    f["all_equal"] = bgzf(lay_sam(h3, [rec(1, 500, "20M", 0, "e%d" % k, pad=5 + k % 7) for k in range(60)]))
    f["strands"] = bgzf(lay_sam(h3, strands()))
    # equal keys in different ingest batches and BGZF blocks: ~230 kB that do not compress, every fifth record of one key
    eq = [rec(1, 777, "20M", 0, "q%d" % k, aux=noise(k, 700)) if k % 5 == 0 else rec(k % 3, 1000 + 37 * (k * 7919 % 300), "20M", 0, "p%d" % k, aux=noise(k, 700))
          for k in range(300)]
    f["eq_batches"] = bgzf(lay_sam(h3, eq))
    f["unplaced_scattered"] = bgzf(lay_sam(h3, shuffled(mixed(14, per=40, unplaced=30), 6)))
    f["unplaced_pos"] = bgzf(lay_sam(h3, shuffled(base + [moved(rec(-1, 0, "", 4, "up%d" % k), p) for k, p in enumerate([5, 0, 700000, 5, -1, 3, 1 << 20])], 7)))
    f["placed_pos_m1"] = bgzf(lay_sam(h3, shuffled(base + [rec(t, -1, "", 4 + 16 * (k & 1), "m%d" % k) for k, t in enumerate([0, 2, 1, 0, 2])], 8)))
    for n in (1, 2, 3, 255, 256, 257):
        rs = np.random.RandomState(100 + n)
        tids = [n - 1, 0, -1, n // 2] + [int(t) for t in rs.randint(-1, n, 40)]
        f["targets_%d" % n] = bgzf(lay_sam(header(refs(n, 1 << 12)), [rec(t, int(rs.randint(0, 4000)) if t >= 0 else -1, "10M" if t >= 0 else "", 0 if t >= 0 else 4, "t%d" % k)
                                                                      for k, t in enumerate(tids)]))
    edge = [moved(rec(0, 0, "10M", 0, "a"), (1 << 29) - 1), moved(rec(0, 0, "10M", 16, "b"), (1 << 30) - 2), moved(rec(0, 0, "10M", 0, "c"), (1 << 30) - 2),
            rec(1, 5, "10M", 0, "d"), rec(0, 7, "10M", 0, "e")]
    f["pos_edges_in"] = bgzf(lay_sam(header(refs(3, (1 << 31) - 1)), edge))
    for name, pos in (("pos_out_2p30m1", (1 << 30) - 1), ("pos_out_m2", -2), ("pos_out_2p31m1", (1 << 31) - 1)):
        out = [moved(r, pos) for r in [rec(1, 0, "10M", 16 * (k & 1), "o%d" % k) for k in range(3)] + [rec(0, 0, "10M", 0, "o3"), rec(-1, 0, "", 4, "o4")]]
        f[name] = bgzf(lay_sam(header(refs(3, (1 << 31) - 1)), shuffled(base + out, 9)))
    f["tid_beyond"] = bgzf(lay_sam(h3, shuffled(base[:40] + [rec(7, 10, "10M", 0, "far"), rec(3, 9, "10M", 0, "near")], 10)))
    f["tid_below"] = bgzf(lay_sam(h3, shuffled(base[:40] + [rec(-5, 10, "", 4, "low"), rec(-2, 9, "", 4, "lower"), rec(-1, -1, "", 4, "u")], 11)))
    f["residues"] = bgzf(lay_sam(h3, residues()))
    big = [sized(0, 900, FULL, "full"), sized(0, 800, FULL + 1, "over"), sized(1, 5, 70000, "big")] + base[:30]
    f["oversize"] = bgzf(lay_sam(h3, shuffled(big, 12)))
    a, c = rec(0, 10, "10M", 0, "first"), rec(0, 30, "10M", 0, "third")
    f["exact_fill"] = bgzf(lay_sam(h3, [c, sized(0, 20, FULL - len(a), "fills"), a]))
    few = shuffled(base[:60], 13)
    f["hd_none"] = bgzf(lay_sam(header(refs(3), text_with("")), few))
    f["hd_no_so"] = bgzf(lay_sam(header(refs(3), text_with("@HD\tVN:1.4\n")), few))
    f["hd_unsorted"] = bgzf(lay_sam(header(refs(3), text_with("@HD\tVN:1.4\tSO:unsorted\n")), few))
    f["hd_so_then_field"] = bgzf(lay_sam(header(refs(3), text_with("@HD\tSO:coordinate\tVN:1.4\n")), few))
    f["hd_so_prefix"] = bgzf(lay_sam(header(refs(3), text_with("@HD\tVN:1.4\tSO:coord\n")), few))
    f["hd_empty_text"] = bgzf(lay_sam(header(refs(3), ""), few))
    f["hd_long"] = bgzf(lay_sam(header(refs(3), text_with(HD_SORTED) + "".join("@CO\tline %d of a header longer than one block\n" % k for k in range(1700))), few))
    st = strands()
    f["packed_97"] = bgzf(lay_packed(h3, st[:150], 97))
    f["packed_1000"] = bgzf(lay_packed(h3, st, 1000))
    f["no_eof"] = bgzf(lay_sam(h3, few), eof=False)
    whole = bgzf(lay_sam(h3, st))
    f["trunc_bytes"] = whole[:len(whole) * 2 // 3]
    s = h3 + b"".join(few[:30])
    f["trunc_stream"] = bgzf([s[:2000], s[2000:len(s) - 17]])
    return f


def materialize(directory):
    """writes every input as NAME.bam under `directory`; returns {file name: sha256}"""
    digests = {}
    for name, data in own_inputs().items():
        with open(os.path.join(directory, name + ".bam"), "wb") as fh:
            fh.write(data)
        digests[name + ".bam"] = hashlib.sha256(data).hexdigest()
    return digests


def names():
    return sorted(own_inputs())


def path_of(name, made):
    return os.path.join(made, name + ".bam")
