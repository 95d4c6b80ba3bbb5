"""CPU: the record-layout tooling of tests/test_bam_raw_layouts_gpu.py and the device index's algorithm on those layouts.

* bamio.BamRecord carries auxiliary fields; write_bam / repack_bam / read_bam_records step over them by block_size;
* tests/bam_layouts.encode_stream (vectorised) writes records the pure-Python decoder reads back as the SoA they came from, in
  samtools' block layout, htsjdk's, and with record chains embedded in aux payloads;
* scripts/emu_raw_chain.py (what kernels/bam_raw.hip does: guess per block, walk, prove, carry) indexes every record of those
  streams over a seeded sample of cuts, cuts inside a record larger than 64 KiB among them."""
import gzip
import os
import struct
import sys

import numpy as np
import pytest

import bam_layouts as BL
from bam_synth import make_soa
from highperformancengs_amd import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FAR_CIGARS = ["150M", "50M2047N50M", "10M20000N10M30000N10M", "5M100000D5M", "40M2I108M", "10S140M", "17000M", "1N1M"]


def test_bam_record_aux_is_written_and_stepped_over(tmp_path):
    rng = np.random.default_rng(3)
    refs = [("c", 100_000)]
    recs = []
    for i in range(300):
        aux = BL.aux_blob(rng, [-1, 0, 5, 40, 3000, 70_000][i % 6])
        seq = "".join("ACGTN"[k] for k in rng.integers(0, 5, 1 + i % 151))
        recs.append(bamio.BamRecord(tid=0, pos=100 * i, flag=[0, 16][i % 2], cigar=bamio.parse_cigar("%dM" % len(seq)), seq=seq,
                                    name="q%d" % i, aux=aux))
    path = str(tmp_path / "a.bam")
    assert bamio.write_bam(path, refs, recs, level=1) == 300
    soa = bamio.read_bam_records(path)
    assert soa.names == [r.name for r in recs] and soa.pos.tolist() == [r.pos for r in recs]
    assert soa.l_qseq.tolist() == [len(r.seq) for r in recs]
    data = gzip.open(path).read()
    o, k = BL.header_len(data), 0
    while o < len(data):                                  # block_size covers the aux bytes, which lie behind the qualities
        bs = struct.unpack_from("<i", data, o)[0]
        assert data[o + 4 + bs - len(recs[k].aux):o + 4 + bs] == recs[k].aux
        o += 4 + bs
        k += 1
    assert k == 300
    bamio.repack_bam(path, str(tmp_path / "p.bam"), 777)
    assert gzip.open(str(tmp_path / "p.bam")).read() == data
    assert BL.same_records(soa, bamio.read_bam_records(str(tmp_path / "p.bam")))


def test_aux_pool_has_every_type():
    pool = BL.aux_pool(1, BL.POOL_SIZES)
    types = set()
    for blob in pool:
        o = 0
        while o < len(blob):                               # parse: every field well formed, back to back
            t = chr(blob[o + 2])
            o += 3
            if t in "AcC":
                o += 1
            elif t in "sS":
                o += 2
            elif t in "iIf":
                o += 4
            elif t in "ZH":
                o = blob.index(b"\0", o) + 1
            else:
                assert t == "B"
                sub = chr(blob[o])
                t += sub
                cnt = struct.unpack_from("<i", blob, o + 1)[0]
                o += 5 + cnt * {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[sub]
            types.add(t)
        assert o == len(blob)
    assert types == set(BL.AUX_TYPES)
    assert max(len(b) for b in pool) >= 30_000


def _cases():
    return {
        "far": lambda: make_soa(6_000, [("chrA", 1_500_000), ("chrB", 200_000)], 31, cigars=FAR_CIGARS, max_start_frac=0.9),
        "ncigar": BL.ncigar_soa,
        "lattice": BL.lattice_soa,
        "long": BL.long_read_soa,
        "big": BL.big_record_soa,
    }


@pytest.mark.parametrize("case", ["far", "ncigar", "lattice", "long", "big", "chain"])
def test_encoder_round_trip_on_every_layout(case):
    soa = _cases()["far" if case == "chain" else case]()
    n = len(soa.tid)
    names = BL.cycling_names(n)
    aux = BL.embedded_chain_aux(5, n) if case == "chain" else BL.pick_aux(5, n)
    data, bounds = BL.encode_stream(soa, names, aux, qual_seed=5)
    assert len(bounds) == n + 1 and bounds[-1] == len(data)
    back = BL.decode_stream(data)
    assert BL.same_records(soa, back)
    assert back.names == [bytes(names[0][names[1][i]:names[1][i + 1]]).decode() for i in range(n)]
    assert {len(s) for s in back.names} >= ({1, 254} if n >= 254 else {1})
    # samtools' layout: blocks of at most 0xff00 bytes, each beginning at a record unless it continues an oversize one
    raw = BL.pack_samtools(data, bounds)
    assert BL.inflate(raw) == data
    at, rec = 0, set(bounds.tolist())
    for _, _, isz in BL.blocks(raw):
        assert isz <= BL.SAMTOOLS_BLOCK
        k = int(np.searchsorted(bounds, at, "right")) - 1
        assert at in rec or at < bounds[0] or (k >= 0 and bounds[k + 1] - bounds[k] > BL.SAMTOOLS_BLOCK)
        at += isz
    for block in (97, 20_000):
        raw = BL.bgzf_pack(data, block, level=1)
        assert BL.inflate(raw) == data and all(isz == block for _, _, isz in BL.blocks(raw)[:-1])


def test_encoder_is_vectorised():
    """10^5 records and more: no Python loop per record"""
    import time
    soa = make_soa(300_000, [("chrA", 30_000_000)], 9)
    t = time.perf_counter()
    data, bounds = BL.encode_stream(soa, BL.cycling_names(300_000), BL.pick_aux(9, 300_000))
    assert time.perf_counter() - t < 30 and len(bounds) == 300_001


def _emu_cuts(data, bounds, blocks, cuts):
    """E.index over two calls cut at block `cut` (blocks: (stream offset, length) of the blocks from the first record's on)"""
    import emu_raw_chain as E
    rec = bounds.tolist()
    hl = rec[0]
    for cut in cuts:
        a0 = blocks[0][0]
        a1 = blocks[cut][0]
        f, n, tail, offs = E.index(data[a0:a1], [(o - a0, ln) for o, ln in blocks[:cut]], hl - a0)
        n_a = int(np.searchsorted(bounds, a1, "right")) - 1
        assert f & 3 == 0 and n == n_a and tail == a1 - rec[n_a] and offs == [r - a0 for r in rec[:n_a]], cut
        front = data[a1 - tail:a1]
        f2, n2, t2, offs2 = E.index(front + data[a1:], [(tail + o - a1, ln) for o, ln in blocks[cut:]], 0)
        assert f2 & 3 == 0 and t2 == 0 and n2 == len(rec) - 1 - n_a, cut
        assert [r + a1 - tail for r in offs2] == rec[n_a:-1], cut


def _stream_blocks(data, bounds, layout):
    raw = BL.pack_samtools(data, bounds, eof=False) if layout == "samtools" else BL.bgzf_pack(data, layout, level=1)
    out, at = [], 0
    for _, _, isz in BL.blocks(raw):
        if at + isz > bounds[0]:
            out.append((at, isz))
        at += isz
    return out


@pytest.mark.parametrize("case,layout", [("big", "samtools"), ("big", 20_000), ("long", "samtools"),
                                         ("chain", 1000), ("lattice", 97)])
def test_guess_walk_prove_and_carry_on_the_new_layouts(case, layout):
    soa = _cases()["far" if case == "chain" else case]()
    if case == "chain":
        soa = make_soa(1500, [("chrA", 900_000)], 71, cigars=["150M", "10S140M", "50M2048N50M"])
    n = len(soa.tid)
    aux = BL.embedded_chain_aux(7, n) if case == "chain" else BL.pick_aux(7, n)
    data, bounds = BL.encode_stream(soa, BL.cycling_names(n), aux, qual_seed=7)
    blocks = _stream_blocks(data, bounds, layout)
    rng = np.random.default_rng(len(blocks))
    cuts = set(int(x) for x in rng.integers(1, len(blocks), 5))
    big = np.flatnonzero(np.diff(bounds) > 65536)
    for r in big[:2]:                                      # calls that end inside a record larger than 64 KiB
        cuts |= {k for k, (o, ln) in enumerate(blocks) if bounds[r] < o < bounds[r + 1]}
    if case == "big":
        assert len(big) and any(bounds[big[0]] < blocks[k][0] for k in cuts)
    _emu_cuts(data, bounds, blocks, sorted(cuts))
