"""bamSplitChr restated in Python: partition + cut rule + framing (bamSplitChr.c:129-138 over samtools-0.1.19's bam_fetch,
bam_write1 and bgzf.c), and the tool's domain decided from the input alone.  tests/test_split_golden.py holds it to the recorded
runs of the compiled reference (tests/golden/split/manifest.json); the GPU tests hold the tool and the ABI to it."""
import gzip
import hashlib
import struct
import zlib

FULL = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Bam:
    """header: the bytes from the magic to the last target's length; names, lens; recs: (tid, pos, bytes with block_size)"""

    def __init__(self, data):
        assert data[:4] == b"BAM\1"
        (l_text,) = struct.unpack_from("<i", data, 4)
        o = 8 + l_text
        (n_ref,) = struct.unpack_from("<i", data, o)
        o += 4
        self.names, self.lens = [], []
        for _ in range(n_ref):
            (l_name,) = struct.unpack_from("<i", data, o)
            self.names.append(data[o + 4:o + 4 + l_name].split(b"\0")[0].decode())
            self.lens.append(struct.unpack_from("<i", data, o + 4 + l_name)[0])
            o += 8 + l_name
        self.header = data[:o]
        self.recs = []
        while o + 4 <= len(data):
            (bs,) = struct.unpack_from("<i", data, o)
            if bs < 32 or o + 4 + bs > len(data):
                break
            tid, pos = struct.unpack_from("<ii", data, o + 4)
            self.recs.append((tid, pos, data[o:o + 4 + bs]))
            o += 4 + bs


def read(path):
    with gzip.open(path, "rb") as fh:
        return Bam(fh.read())


def first_offender(bam):
    """(ordinal, tid, pos, reason) of the first record outside the domain, or None -- the rules of kernels/bam_split.hip"""
    n_ref, prev = len(bam.names), None
    for i, (tid, pos, _) in enumerate(bam.recs):
        reason = 0
        if tid < -1 or tid >= n_ref:
            reason = 1
        elif tid >= 0 and not 0 <= pos < 1 << 29:
            reason = 2
        elif prev is not None and (tid & 0xffffffff) < (prev[0] & 0xffffffff):
            reason = 3
        elif prev is not None and tid == prev[0] and tid >= 0 and pos < prev[1]:
            reason = 4
        if reason:
            return i, tid, pos, reason
        prev = (tid, pos)
    return None


def index_fault(bai, bam):
    """what of the index puts the input outside the domain, or None: magic, n_ref, the pseudo-bins' record counts"""
    if bai[:4] != b"BAI\1":
        return "magic"
    (n,) = struct.unpack_from("<i", bai, 4)
    if n != len(bam.names):
        return "n_ref"
    counts = [0] * n
    for tid, _, _ in bam.recs:
        if 0 <= tid < n:
            counts[tid] += 1
    o = 8
    for t in range(n):
        (n_bin,) = struct.unpack_from("<i", bai, o)
        o += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, o)
            o += 8
            if b == 37450 and n_chunk == 2:
                mapped, unmapped = struct.unpack_from("<QQ", bai, o + 16)
                if mapped + unmapped != counts[t]:
                    return "pseudo-bin"
            o += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", bai, o)
        o += 4 + 8 * n_intv
    return None


def classify(bam, bai, prefix):
    """None inside the domain, else ("record", ordinal, tid, pos, reason) / ("index", what) / ("name", target)"""
    f = index_fault(bai, bam)
    if f:
        return ("index", f)
    for t, name in enumerate(bam.names):
        if len(prefix) + 1 + len(name.encode()) + 4 >= 256:
            return ("name", t)
    bad = first_offender(bam)
    return ("record",) + bad if bad else None


def cut(records):
    """bam_write1 per record: bgzf_flush_try(4 + block_len), then bgzf_write -- the payloads of the blocks"""
    out, blk = [], bytearray()
    for r in records:
        if len(blk) + len(r) > FULL:
            if blk:
                out.append(bytes(blk))
            blk = bytearray()
        at = 0
        while at < len(r):
            k = min(FULL - len(blk), len(r) - at)
            blk += r[at:at + k]
            at += k
            if len(blk) == FULL:
                out.append(bytes(blk))
                blk = bytearray()
    if blk:
        out.append(bytes(blk))
    return out


def member(payload, level):
    """one block as bgzf.c's deflate_block makes it: deflate() in ONE Z_FINISH call -- at level 0 that is one final stored block,
    01 LEN NLEN (compressobj's compress() + flush() are two calls and end with an empty stored block of their own)"""
    if level == 0:
        comp = b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload
    else:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        comp = co.compress(payload) + co.flush()
    return (struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def payloads(bam):
    """per target: the payloads of its file's blocks (header first), and its record count"""
    head = [bam.header[i:i + FULL] for i in range(0, len(bam.header), FULL)]
    out = []
    for t in range(len(bam.names)):
        recs = [r for tid, _, r in bam.recs if tid == t]
        out.append((head + cut(recs), len(recs)))
    return out


def split(bam, level=-1):
    """[(target name, file bytes, record count)] in header order"""
    return [(bam.names[t], b"".join(member(p, level) for p in pl) + EOF_BLOCK, n) for t, (pl, n) in enumerate(payloads(bam))]


def blocks_of(data):
    """a BGZF file -> [(payload, crc field, whole block bytes)], the 28-byte EOF block included"""
    out, o = [], 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 12:o + 14] == b"BC", o
        xlen, = struct.unpack_from("<H", data, o + 10)
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", data, o + bsize - 8)
        payload = zlib.decompress(data[o + 12 + xlen:o + bsize - 8], -15)
        assert len(payload) == isize and zlib.crc32(payload) & 0xffffffff == crc, o
        out.append((payload, crc, data[o:o + bsize]))
        o += bsize
    return out


def describe(data):
    """what the manifest keeps of an output file"""
    bl = blocks_of(data)
    return {"size": len(data), "sha256": hashlib.sha256(data).hexdigest(), "isize": [len(p) for p, _, _ in bl], "inflated_sha256": hashlib.sha256(b"".join(p for p, _, _ in bl)).hexdigest()}


def stderr_of(bam, inputs):
    """the reference's lines with the times masked, for one input path"""
    return "".join("chr: %s\tchr_len: %d\treads_count: %d at T s\n" % (n, l, sum(1 for tid, _, _ in bam.recs if tid == t))
                   for t, (n, l) in enumerate(zip(bam.names, bam.lens))) + "splited %s into each chromosome at T s\n" % inputs
