"""Record layouts of real-world BAM files for the tests of the in-place record route (kernels/bam_raw.hip, RawRecs of
kernels/bam_depth.hip, k_raw_fields + kernels/bam_window.hip): read names of 1 .. 254 characters, auxiliary fields of every
SAM type (B arrays up to tens of kB), CIGARs of up to 65,535 operations, long reads -- and the three ways a BAM's
uncompressed stream is cut into BGZF blocks:

* samtools' (record-aligned blocks of up to 0xff00 bytes, an oversize record in a run of blocks of its own: bamio._Bgzf);
* htsjdk's (fixed-size blocks wherever they fall, records running across block ends: bgzf_pack);
* a stream whose aux payloads embed a well-formed chain of real record bytes (chain_aux): a block that starts inside such a
  payload finds a plausible first record that is none, and only the proof of the chain may refute it.

encode_stream is vectorised (numpy gathers, no Python loop per record): it takes the test SoAs of 10^5 records and more."""
import struct
import zlib

import numpy as np

from highperformancengs_amd import bamio

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SAMTOOLS_BLOCK = 0xFF00

# ---- BGZF blocks ----------------------------------------------------------------------------------------------------


def bgzf_member(piece, level=1):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(piece) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (len(comp) + 25).to_bytes(2, "little") + comp +
            (zlib.crc32(piece) & 0xffffffff).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))


def blocks(raw):
    """BGZF member chain -> list of (payload_off, payload_len, isize)"""
    out, o = [], 0
    while o < len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append((o + 12 + xlen, bsize - xlen - 20, struct.unpack_from("<I", raw, o + bsize - 4)[0]))
        o += bsize
    return out


def inflate(raw):
    return b"".join(zlib.decompress(raw[a:a + n], -15) for a, n, _ in blocks(raw))


def header_len(text):
    l_text = struct.unpack_from("<i", text, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", text, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", text, p)[0]
    return p


def bgzf_pack(data, block, level=6, eof=False):
    """htsjdk's layout: the stream cut into blocks of `block` bytes wherever that falls"""
    return b"".join(bgzf_member(data[i:i + block], level) for i in range(0, len(data), block)) + (BGZF_EOF if eof else b"")


def pack_samtools(data, bounds, level=1, eof=True):
    """samtools' layout (bam.c:238 bgzf_flush_try; bamio._Bgzf): the header in blocks of its own, then as many whole records
    to a block as fit in 0xff00 bytes; a record larger than that in a run of blocks of its own.  bounds: record starts + end."""
    bounds = np.asarray(bounds, np.int64)
    out = [bgzf_member(data[i:min(i + SAMTOOLS_BLOCK, int(bounds[0]))], level) for i in range(0, int(bounds[0]), SAMTOOLS_BLOCK)]
    k = 0
    while k + 1 < len(bounds):
        j = int(np.searchsorted(bounds, bounds[k] + SAMTOOLS_BLOCK, "right")) - 1
        if j <= k:                                          # an oversize record
            a, b = int(bounds[k]), int(bounds[k + 1])
            out += [bgzf_member(data[i:min(i + SAMTOOLS_BLOCK, b)], level) for i in range(a, b, SAMTOOLS_BLOCK)]
            k += 1
        else:
            out.append(bgzf_member(data[int(bounds[k]):int(bounds[j])], level))
            k = j
    return b"".join(out) + (BGZF_EOF if eof else b"")


def to_device(ctx, raw):
    """BGZF file bytes -> (d_raw, info, keepalive): the blocks from the one holding the first record on, inflated on the device
    (hpn_bgzf_inflate_dev), the records indexed where they lie (hpn_bam_raw_index_dev)"""
    import torch
    blks = blocks(raw)
    text, hl = b"", None
    for a, n, _ in blks:                                    # as many blocks as the header takes (tiny blocks: several)
        text += zlib.decompress(raw[a:a + n], -15)
        try:
            hl = header_len(text)
            break
        except struct.error:
            continue
    first, acc = 0, 0
    while acc + blks[first][2] <= hl and first < len(blks) - 1:  # the block the header ends in (or the next one)
        acc += blks[first][2]
        first += 1
    blks = blks[first:]
    table = np.zeros((len(blks), 3), np.uint64)
    outo = 0
    for i, (a, n, isz) in enumerate(blks):
        table[i] = (a, n | (isz << 32), outo)
        outo += isz
    d_comp = torch.from_numpy(np.frombuffer(raw + bytes(64), np.uint8).copy()).cuda()
    d_blocks = torch.from_numpy(table.view(np.int64)).cuda()
    d_out = torch.zeros(outo + 64, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(len(blks), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.bgzf_inflate_dev(d_comp, d_blocks, len(blks), d_out, d_status)
    info = ctx.bam_raw_index_dev(d_out, d_blocks, len(blks), hl - acc, d_status)
    return d_out, info, (d_comp, d_blocks, d_status)


# ---- record bytes -----------------------------------------------------------------------------------------------------

_FIXED = np.dtype([("bs", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                   ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("tlen", "<i4")])
assert _FIXED.itemsize == 36
_NAME_CHARS = np.frombuffer(bytes(c for c in range(33, 127) if c != 64) * 4, np.uint8)   # SAM QNAME [!-?A-~]


def _gather(src, s_off, lens):
    """src[s_off[i] : s_off[i] + lens[i]] for every i, back to back"""
    lens = np.asarray(lens, np.int64)
    tot = int(lens.sum())
    if tot == 0:
        return np.zeros(0, src.dtype)
    fs = np.cumsum(lens) - lens
    return src[np.arange(tot, dtype=np.int64) + np.repeat(np.asarray(s_off, np.int64) - fs, lens)]


def _place(out, d_off, flat, lens):
    """out[d_off[i] : d_off[i] + lens[i]] = the i-th piece of flat"""
    lens = np.asarray(lens, np.int64)
    tot = int(lens.sum())
    if tot == 0:
        return
    fs = np.cumsum(lens) - lens
    out[np.arange(tot, dtype=np.int64) + np.repeat(np.asarray(d_off, np.int64) - fs, lens)] = flat


def ragged(pieces):
    """list of bytes -> (flat uint8, off int64[n + 1])"""
    off = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    return np.frombuffer(b"".join(pieces), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8), off


def cycling_names(n, lo=1, hi=254):
    """read names of lo .. hi characters, one length after the other (l_read_name lo + 1 .. hi + 1)"""
    lens = lo + np.arange(n, dtype=np.int64) % (hi - lo + 1)
    s = np.arange(n, dtype=np.int64) % 97
    flat = _gather(_NAME_CHARS, s, lens)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return flat, off


def _ref_len(soa):
    """bam_calend's span (M D N = X) per record, vectorised"""
    cig = soa.cigar.astype(np.int64)
    op, ln = cig & 0xF, cig >> 4
    ref = np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0)
    cs = np.concatenate([[0], np.cumsum(ref)])
    return cs[soa.cigar_off[1:].astype(np.int64)] - cs[soa.cigar_off[:-1].astype(np.int64)]


def _reg2bin(beg, end):
    end = end - 1
    out = np.zeros(len(beg), np.int64)
    done = np.zeros(len(beg), bool)
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        hit = ~done & ((beg >> shift) == (end >> shift))
        out[hit] = base + (beg[hit] >> shift)
        done |= hit
    return out


def header_bytes(refs, text=None):
    if text is None:
        text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, ln) for nm, ln in refs)
    ht = text.encode()
    hdr = b"BAM\1" + struct.pack("<i", len(ht)) + ht + struct.pack("<i", len(refs))
    for nm, ln in refs:
        nb = nm.encode() + b"\0"
        hdr += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    return hdr


def encode_stream(soa, names=None, aux=None, qual_seed=0, chunk=1 << 15):
    """BamSoA (+ names, aux as (flat, off) ragged arrays) -> (uncompressed BAM stream: header + records, bounds int64[n + 1]:
    the stream offset of every record and of the end).  Qualities are random bytes (what follows a sequence is no padding)."""
    n = len(soa.tid)
    hdr = header_bytes(soa.refs)
    if names is None:
        names = (np.frombuffer(b"r" * n, np.uint8).copy(), np.arange(n + 1, dtype=np.int64))
    if aux is None:
        aux = (np.zeros(0, np.uint8), np.zeros(n + 1, np.int64))
    nf, no = names
    af, ao = aux
    name_len = np.diff(no)
    assert name_len.max(initial=1) <= 254 and name_len.min(initial=1) >= 1
    n_cig = np.diff(soa.cigar_off.astype(np.int64))
    assert n_cig.max(initial=0) <= 65535
    l_seq = soa.l_qseq.astype(np.int64)
    nb = (l_seq + 1) // 2
    a_len = np.diff(ao)
    bs = 32 + (name_len + 1) + 4 * n_cig + nb + l_seq + a_len
    bounds = np.zeros(n + 1, np.int64)
    np.cumsum(4 + bs, out=bounds[1:])
    bounds += len(hdr)
    out = np.zeros(int(bounds[-1]), np.uint8)
    out[:len(hdr)] = np.frombuffer(hdr, np.uint8)
    pos = soa.pos.astype(np.int64)
    rl = _ref_len(soa) if n else np.zeros(0, np.int64)
    bins = np.where(pos >= 0, _reg2bin(np.maximum(pos, 0), np.maximum(pos, 0) + np.maximum(rl, 1)), 4680)
    fx = np.zeros(n, _FIXED)
    fx["bs"], fx["tid"], fx["pos"], fx["l_name"], fx["mapq"] = bs, soa.tid, soa.pos, name_len + 1, 30
    fx["bin"], fx["n_cigar"], fx["flag"], fx["l_seq"] = bins, n_cig, soa.flag, l_seq
    fx["mtid"], fx["mpos"], fx["tlen"] = -1, -1, 0
    cig8 = soa.cigar.view(np.uint8)
    rng = np.random.default_rng(qual_seed)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        r0 = bounds[a:b]
        _place(out, r0, fx[a:b].view(np.uint8), np.full(b - a, 36))
        q = r0 + 36
        _place(out, q, _gather(nf, no[a:b], name_len[a:b]), name_len[a:b])
        q = q + name_len[a:b] + 1                                    # (+ the NUL: out is zeros)
        _place(out, q, _gather(cig8, 4 * soa.cigar_off[a:b].astype(np.int64), 4 * n_cig[a:b]), 4 * n_cig[a:b])
        q = q + 4 * n_cig[a:b]
        _place(out, q, _gather(soa.seq4, soa.seq_off[a:b].astype(np.int64), nb[a:b]), nb[a:b])
        q = q + nb[a:b]
        _place(out, q, rng.integers(0, 256, int(l_seq[a:b].sum()), dtype=np.uint8), l_seq[a:b])
        q = q + l_seq[a:b]
        _place(out, q, _gather(af, ao[a:b], a_len[a:b]), a_len[a:b])
    return out.tobytes(), bounds


def decode_stream(data):
    """the pure-Python decoder (bamio.read_bam_records) on an uncompressed stream"""
    import gzip
    import os
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".bam")
    try:
        with os.fdopen(fd, "wb") as fh:
            fh.write(gzip.compress(data, 1))
        return bamio.read_bam_records(path)
    finally:
        os.unlink(path)


# ---- auxiliary fields -----------------------------------------------------------------------------------------------

_B_SUB = {"c": ("b", 1), "C": ("B", 1), "s": ("h", 2), "S": ("H", 2), "i": ("i", 4), "I": ("I", 4), "f": ("f", 4)}


def aux_field(rng, typ, size=8):
    """one aux field of SAM type typ (A c C s S i I f Z H, or B + subtype: "Bc" .. "Bf") with a payload of about `size` bytes"""
    tag = bytes([rng.integers(65, 91), rng.integers(48, 58) if rng.random() < 0.5 else rng.integers(65, 91)])
    if typ == "A":
        return tag + b"A" + bytes([rng.integers(33, 127)])
    if typ in ("c", "C", "s", "S", "i", "I"):
        f, w = _B_SUB[typ]
        lo, hi = {"b": (-128, 128), "B": (0, 256), "h": (-32768, 32768), "H": (0, 65536), "i": (-2 ** 31, 2 ** 31), "I": (0, 2 ** 32)}[f]
        return tag + typ.encode() + struct.pack("<" + f, int(rng.integers(lo, hi)))
    if typ == "f":
        return tag + b"f" + struct.pack("<f", float(rng.standard_normal()))
    if typ == "Z":
        return tag + b"Z" + bytes(rng.integers(32, 127, max(size, 0)).astype(np.uint8)) + b"\0"
    if typ == "H":
        return tag + b"H" + bytes(rng.choice(np.frombuffer(b"0123456789ABCDEF", np.uint8), 2 * max(size // 2, 0))) + b"\0"
    f, w = _B_SUB[typ[1]]
    cnt = max(size // w, 0)
    if f == "f":
        vals = rng.standard_normal(cnt).astype("<f4").tobytes()
    else:
        vals = rng.integers(0, 256, cnt * w, dtype=np.uint8).tobytes()
    return tag + b"B" + typ[1].encode() + struct.pack("<i", cnt) + vals


AUX_TYPES = ["A", "c", "C", "s", "S", "i", "I", "f", "Z", "H", "Bc", "BC", "Bs", "BS", "Bi", "BI", "Bf"]


def aux_blob(rng, size):
    """aux fields about `size` bytes in all (0: none; -1: one field of every type, the B arrays of 0 .. 3 elements)"""
    if size < 0:
        return b"".join(aux_field(rng, t, k % 4 * 4) for k, t in enumerate(AUX_TYPES))
    if size == 0:
        return b""
    out = b""
    k = int(rng.integers(0, len(AUX_TYPES)))
    while len(out) < size:
        typ = AUX_TYPES[k % len(AUX_TYPES)]
        out += aux_field(rng, typ, int(min(size - len(out), rng.integers(0, 64) if len(typ) == 1 else size)))
        k += 1
    return out


def aux_pool(seed, sizes):
    rng = np.random.default_rng(seed)
    return [aux_blob(rng, s) for s in sizes]


# a pool of mostly small blobs (NM/MD/AS/RG-like), a few of kilobytes (MM/ML) and rare ones of tens of kB
POOL_SIZES = [-1, 0, 3, 7, 12, 16, 20, 31, 33, 40, 47, 60, 64, 90, 128, 200, 255, 500, 1024, 4096, 9000, 30000]
POOL_P = np.array([8, 8, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 4, 4, 3, 3, 2, 1, 0.4, 0.2, 0.05])


def pick_aux(seed, n, pool=None, p=None):
    """(flat, off) aux for n records drawn from a pool of blobs, vectorised"""
    pool = pool if pool is not None else aux_pool(seed, POOL_SIZES)
    p = POOL_P if p is None else np.asarray(p, np.float64)
    rng = np.random.default_rng(seed + 1)
    k = rng.choice(len(pool), size=n, p=p / p.sum())
    pf, po = ragged(pool)
    lens = np.diff(po)[k]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return _gather(pf, po[k], lens), off


def chain_aux(seed, n_rec=6, tid=0, pos=100):
    """a B:C array holding the bytes of n_rec well-formed records with printable names (a four-in-a-row chain k_raw_starts would
    take for a block's first record) -- embedded in a record, it must never be indexed"""
    refs = [("c", 1 << 20)]
    from bam_synth import make_soa
    fake = make_soa(n_rec, refs, seed, cigars=["20M", "5M3I12M", "30M"])
    fake.tid[:] = tid
    fake.pos[:] = pos + np.arange(n_rec)
    nf, no = cycling_names(n_rec, 4, 30)
    data, bounds = encode_stream(fake, names=(nf, no), qual_seed=seed)
    payload = data[int(bounds[0]):]
    return b"XCBC" + struct.pack("<i", len(payload)) + payload


def embedded_chain_aux(seed, n, every=7):
    """(flat, off) aux for n records: every `every`-th record carries a chain_aux, the others a small blob"""
    small = aux_pool(seed, [0, 5, 17, 40])
    chains = [chain_aux(seed + k, n_rec=5 + k % 4, pos=1000 * k) for k in range(8)]
    pieces = [chains[(i // every) % 8] if i % every == 3 else small[i % 4] for i in range(min(n, 4096))]
    pf, po = ragged(pieces)
    k = np.arange(n) % len(pieces)
    lens = np.diff(po)[k]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return _gather(pf, po[k], lens), off


# ---- SoA helpers --------------------------------------------------------------------------------------------------


def soa_from(refs, recs):
    """BamSoA from (tid, pos, flag, cigar text or packed list, l_seq, seq4 bytes or None) tuples"""
    cig = [bamio.parse_cigar(c) if isinstance(c, str) else list(c) for _, _, _, c, _, _ in recs]
    seqs = [s if s is not None else bytes((lq + 1) // 2) for _, _, _, _, lq, s in recs]
    for (_, _, _, _, lq, _), s in zip(recs, seqs):
        assert len(s) == (lq + 1) // 2
    coff = np.zeros(len(recs) + 1, np.uint32)
    np.cumsum([len(c) for c in cig], out=coff[1:])
    soff = np.zeros(len(recs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=soff[1:])
    return bamio.BamSoA(refs=list(refs), tid=np.array([r[0] for r in recs], np.int32), pos=np.array([r[1] for r in recs], np.int32),
                        flag=np.array([r[2] for r in recs], np.uint32), l_qseq=np.array([r[4] for r in recs], np.int32),
                        cigar_off=coff, cigar=np.array([w for c in cig for w in c], np.uint32).reshape(-1),
                        seq_off=soff, seq4=np.frombuffer(b"".join(seqs) + b"\0", np.uint8).copy())


def same_records(a, b):
    """the fields the kernels read, record for record (sequence bytes through each record's own offsets)"""
    if len(a.tid) != len(b.tid):
        return False
    for f in ("tid", "pos", "flag", "l_qseq"):
        if not np.array_equal(getattr(a, f).astype(np.int64), getattr(b, f).astype(np.int64)):
            return False
    na, nb_ = np.diff(a.cigar_off.astype(np.int64)), np.diff(b.cigar_off.astype(np.int64))
    if not np.array_equal(na, nb_):
        return False
    if not np.array_equal(_gather(a.cigar, a.cigar_off[:-1], na), _gather(b.cigar, b.cigar_off[:-1], nb_)):
        return False
    ln = (a.l_qseq.astype(np.int64) + 1) // 2
    return np.array_equal(_gather(a.seq4, a.seq_off[:-1], ln), _gather(b.seq4, b.seq_off[:-1], ln))


# ---- record sets only the in-place route has to get right -------------------------------------------------------------

_OPS = "MIDNSHP=X"
N_CIGARS = (0, 1, 2, 3, 4, 5, 16, 255, 1000, 65535)
TAILS = (None, "D", "N", "I", "S")


def _cigar_of(n, tail, rng):
    """n operations whose last M is followed by `tail` (or is the last operation)"""
    m = n - (tail is not None)
    body = []
    for k in range(m):
        if (m - 1 - k) % 2 == 0:
            body.append((int(rng.integers(1, 6)) << 4) | 0)                       # M
        else:
            op = "DNIX="[k % 5]
            body.append((int(rng.integers(1, 50 if op == "N" else 4)) << 4) | _OPS.index(op))
    if tail is not None and n:
        body.append((int(rng.integers(1, 3000 if tail == "N" else 9)) << 4) | _OPS.index(tail))
    return body


def _qlen(cig):
    return sum(w >> 4 for w in cig if (w & 0xF) in (0, 1, 4, 7, 8))


def _rand_seq(rng, lq):
    return rng.integers(0, 256, (lq + 1) // 2, dtype=np.uint8).tobytes()


def ncigar_soa(seed=1):
    """n_cigar in N_CIGARS (0 on a mapped record) with the last M followed or not by D / N / I / S, between 150-base reads"""
    rng = np.random.default_rng(seed)
    refs = [("c", 3_000_000), ("d", 800_000)]
    recs = []
    for t, (_, tlen) in enumerate(refs):
        for p in sorted(int(x) for x in rng.integers(0, tlen // 2, 1500)):
            recs.append((t, p, 0, "150M", 150, _rand_seq(rng, 150)))
    special = []
    for n in N_CIGARS:
        for tail in TAILS:
            if n == 0 and tail is not None:
                continue
            cig = _cigar_of(n, tail, rng)
            lq = _qlen(cig) if n <= 255 else 0
            for t in (0, 1):
                special.append((t, int(rng.integers(0, refs[t][1] // 2)), 0, cig, lq if n else 151,
                                _rand_seq(rng, lq if n else 151)))
    recs += special
    recs.sort(key=lambda r: (r[0], r[1]))
    return soa_from(refs, recs)


LATTICE_GAPS = (2047, 2048, 2049, 10_000, 100_000, 500_000)


def lattice_soa(T=16384):
    """N / D of 2,047 .. 2,049 and 10^4 .. 5 x 10^5: records on the tile lattice (pos = kT - 1, kT, kT + 1) and far breakpoints
    landing on it (pos + 10 + gap = uT - 1, uT, uT + 1)"""
    refs = [("c", 1_200_000)]
    recs = []
    for gap in LATTICE_GAPS:
        for op in "ND":
            cg = "10M%d%s10M" % (gap, op)
            for k in (1, 3, 8):
                for d in (-1, 0, 1):
                    recs.append((0, k * T + d, 0, cg, 20, None))
                    land = (k * T + gap) // T * T + T + d        # the breakpoint after the gap on a tile edge
                    recs.append((0, land - 10 - gap, 0, cg, 20, None))
    recs.sort(key=lambda r: r[1])
    return soa_from(refs, recs)


LONG_LSEQ = (257, 511, 512, 1000, 20_000)


def long_read_soa(seed=3, n=3000):
    """l_seq 257 .. 20,000 and three 70,000-base all-G soft-clipped reads (per-read G/C beyond 65,535) among 150-base reads and
    SEQ * records in the same waves; an odd-length long read last"""
    rng = np.random.default_rng(seed)
    refs = [("chrM", 16_569), ("c", 2_000_000)]
    recs = []
    pos = np.sort(rng.integers(0, 1_900_000, n))
    for i in range(n):
        if i % 7 == 3:
            recs.append((1, int(pos[i]), 0, "150M", 0, None))                    # SEQ *
        elif i % 23 == 5:
            lq = LONG_LSEQ[(i // 23) % len(LONG_LSEQ)]
            recs.append((1, int(pos[i]), 0, "%dM" % lq, lq, _rand_seq(rng, lq)))
        else:
            recs.append((1, int(pos[i]), [0, 16][i % 2], "150M", 150, _rand_seq(rng, 150)))
    allg = bytes([0x44]) * 35_000
    chrm = [(0, p, 0, "100M69900S", 70_000, allg) for p in (100, 150, 16_000)]
    chrm += [(0, p, 0, "150M", 150, _rand_seq(rng, 150)) for p in range(0, 16_400, 250)]
    chrm.sort(key=lambda r: r[1])
    last = (1, 1_950_000, 0, "20001M", 20_001, _rand_seq(rng, 20_001))
    return soa_from(refs, chrm + recs + [last])


def big_record_soa(seed=4):
    """a record of ~240 KB (l_seq 160,000) between short reads: it spans four of samtools' blocks"""
    rng = np.random.default_rng(seed)
    refs = [("c", 500_000)]
    recs = [(0, 1000 + 37 * i, 0, "150M", 150, _rand_seq(rng, 150)) for i in range(600)]
    recs.append((0, 30_000, 0, "60000M100000S", 160_000, _rand_seq(rng, 160_000)))
    recs += [(0, 30_000 + 41 * i, 0, "150M", 150, _rand_seq(rng, 150)) for i in range(600)]
    return soa_from(refs, recs)


# ---- whole BAM files (+ .bai) for the tools -----------------------------------------------------------------------------

def write_bam_file(path, data, bounds, soa, layout, level=1):
    """the stream in `layout` ("samtools" or the htsjdk block size) to path, with a .bai of the virtual offsets of ITS blocks
    (bam_index.c's bins and 16 kb linear index, bamio._write_bai)"""
    raw = pack_samtools(data, bounds, level) if layout == "samtools" else bgzf_pack(data, int(layout), level, eof=True)
    with open(path, "wb") as fh:
        fh.write(raw)
    blks = blocks(raw)
    caddr = np.array([a - 18 for a, _, _ in blks], np.int64)             # (BGZF header: 12 bytes + XLEN 6)
    ustart = np.concatenate([[0], np.cumsum([isz for _, _, isz in blks])]).astype(np.int64)

    def voff(u):
        k = np.searchsorted(ustart, u, "right") - 1
        k = np.minimum(k, len(blks) - 1)
        return (caddr[k] << 16) | (u - ustart[k])
    n = len(soa.tid)
    beg, end = voff(bounds[:-1]), voff(bounds[1:])
    end_u = bounds[1:]
    full = end_u == ustart[np.minimum(np.searchsorted(ustart, end_u, "right") - 1, len(blks) - 1)]
    # a record that ends a block: bgzf_tell reports the next block's address (bgzf.c:342)
    nxt = np.searchsorted(ustart, end_u, "left")
    end = np.where(full & (nxt < len(blks)), caddr[np.minimum(nxt, len(blks) - 1)] << 16, end)
    rl = _ref_len(soa)
    rend = soa.pos.astype(np.int64) + np.maximum(rl, 1)
    bins_of = _reg2bin(np.maximum(soa.pos.astype(np.int64), 0), rend)
    n_ref = len(soa.refs)
    bins = [dict() for _ in range(n_ref)]
    lidx = [dict() for _ in range(n_ref)]
    tid, pos = soa.tid.tolist(), soa.pos.tolist()
    beg, end, bins_of, rend = beg.tolist(), end.tolist(), bins_of.tolist(), rend.tolist()
    for r in range(n):
        t = tid[r]
        if t < 0:
            continue
        ch = bins[t].setdefault(bins_of[r], [])
        if ch and ch[-1][1] == beg[r]:
            ch[-1][1] = end[r]
        else:
            ch.append([beg[r], end[r]])
        li = lidx[t]
        for w in range(pos[r] >> 14, ((rend[r] - 1) >> 14) + 1):
            if w not in li or beg[r] < li[w]:
                li[w] = beg[r]
    bamio._write_bai(path + ".bai", n_ref, bins, lidx)


def rnaseq_soa(n, refs, seed):
    """spliced reads: 100 bases in two or three exons, introns of 1 kb .. 5 x 10^5 (log-uniform), some soft clips"""
    rng = np.random.default_rng(seed)
    tl = np.array([l for _, l in refs], np.int64)
    tid = np.sort(rng.choice(len(refs), n, p=tl / tl.sum()))
    intr = np.exp(rng.uniform(np.log(1000), np.log(500_000), (n, 2))).astype(np.int64)
    three = rng.random(n) < 0.3
    a = rng.integers(5, 60, n)
    b = np.where(three, rng.integers(5, 95 - a), 100 - a)
    c = np.where(three, 100 - a - b, 0)
    clip = np.where(rng.random(n) < 0.2, rng.integers(1, 5, n), 0)
    span = a + intr[:, 0] + b + np.where(three, intr[:, 1] + c, 0)
    pos = (rng.random(n) * np.maximum(tl[tid] - span - 1, 1)).astype(np.int64)
    order = np.lexsort((pos, tid))
    tid, pos, a, b, c, clip, intr, three = tid[order], pos[order], a[order], b[order], c[order], clip[order], intr[order], three[order]
    nops = 3 + 2 * three + (clip > 0)
    coff = np.zeros(n + 1, np.int64)
    np.cumsum(nops, out=coff[1:])
    cig = np.zeros(int(coff[-1]), np.uint32)
    at = coff[:-1].copy()
    hasclip = clip > 0
    cig[at[hasclip]] = (clip[hasclip] << 4) | 4                              # S
    at += hasclip
    cig[at] = ((a - clip) << 4) | 0
    cig[at + 1] = (intr[:, 0] << 4) | 3
    cig[at + 2] = (b << 4) | 0
    cig[(at + 3)[three]] = (intr[three, 1] << 4) | 3
    cig[(at + 4)[three]] = (c[three] << 4) | 0
    lq = np.full(n, 100, np.int32)
    soff = np.zeros(n + 1, np.uint64)
    np.cumsum((lq + 1) // 2, out=soff[1:])
    codes = np.array([1, 2, 4, 8, 15], np.uint8)
    k = rng.integers(0, 4, (int(soff[-1]), 2)) + (rng.random((int(soff[-1]), 2)) < 0.02)
    seq4 = (codes[k[:, 0]] << 4) | codes[k[:, 1]]
    flags = np.array([0, 16, 99, 147, 83, 163, 256, 1024, 4], np.uint32)
    return bamio.BamSoA(refs=list(refs), tid=tid.astype(np.int32), pos=pos.astype(np.int32),
                        flag=flags[rng.integers(0, len(flags), n)], l_qseq=lq, cigar_off=coff.astype(np.uint32), cigar=cig,
                        seq_off=soff, seq4=seq4.astype(np.uint8))


def rnaseq_aux(n, seed):
    """NH HI AS nM MD per record"""
    rng = np.random.default_rng(seed)
    pool = []
    for k in range(64):
        nh = 1 + k % 4
        pool.append(b"NHC" + bytes([nh]) + b"HIC" + bytes([1 + k % nh]) + b"ASC" + bytes([150 + k % 50]) + b"nMC" + bytes([k % 3]) +
                    b"MDZ" + (b"%d" % (k * 7 % 100)) + b"A" + (b"%d" % (k % 50)) + b"\0")
    pf, po = ragged(pool)
    pick = rng.integers(0, len(pool), n)
    lens = np.diff(po)[pick]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return _gather(pf, po[pick], lens), off


def long_read_file_soa(n, refs, seed):
    """reads of 1 .. 100 kb (log-uniform) whose CIGARs hold thousands of operations (M runs with small I / D between)"""
    rng = np.random.default_rng(seed)
    tl = np.array([l for _, l in refs], np.int64)
    recs = []
    for i in range(n):
        t = int(rng.choice(len(refs), p=tl / tl.sum()))
        L = int(np.exp(rng.uniform(np.log(1000), np.log(100_000))))
        n_ops = max(1, L // 40)
        m = rng.integers(10, 60, n_ops)
        gaps = rng.integers(1, 4, n_ops)
        ops = rng.choice([1, 2], n_ops)
        cig = np.empty(2 * n_ops - 1, np.uint32)
        cig[0::2] = (m << 4) | 0
        cig[1::2] = (gaps[:-1] << 4) | ops[:-1]
        ql = int(m.sum() + gaps[:-1][ops[:-1] == 1].sum())
        span = int(m.sum() + gaps[:-1][ops[:-1] == 2].sum())
        p = int(rng.integers(0, tl[t] - span - 1))
        recs.append((t, p, [0, 16][i % 2], cig.tolist(), ql, rng.integers(0, 256, (ql + 1) // 2, dtype=np.uint8).tobytes()))
    recs.sort(key=lambda r: (r[0], r[1]))
    return soa_from(refs, recs)


def long_read_aux(soa, seed):
    """MM / ML: a Z string and a B:C array of about one byte per 20 bases"""
    rng = np.random.default_rng(seed)
    pieces = []
    for lq in soa.l_qseq.tolist():
        k = max(1, lq // 20)
        pieces.append(b"MMZC+m?," + b",".join(b"%d" % v for v in rng.integers(0, 30, min(k, 2000))) + b";\0" +
                      b"MLBC" + struct.pack("<i", k) + rng.integers(0, 256, k, dtype=np.uint8).tobytes())
    return ragged(pieces)
