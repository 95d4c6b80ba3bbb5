"""What `samtools index` of samtools-0.1.19 makes of a BAM file, restated sequentially: the BGZF reader's view of the file (which
virtual offset it reports after every read), the chunk runs, the merge inside a bin's list, the linear index with its length,
the metadata bin 37450, the order in which the hash table of a target hands out its bins, and the messages.  The recorded runs
of tests/golden/bai/manifest.json pin it to the compiled reference (tests/test_bai_golden.py); the tool's host route
(csrc/host/bai_build.hpp) and the device route are held to the same recordings.

index(data) -> (bai bytes or None, stderr text).  Refuse is raised where the reference's behaviour is undefined (a refID outside
the header's targets, a record whose name and CIGAR do not fit its size, a mapped record with a negative position, a header
that ends early): the tool leaves with status 2 there."""
import struct
import zlib

META_BIN = 37450
PRIMES = [0, 3, 11, 23, 53, 97, 193, 389, 769, 1543, 3079, 6151, 12289, 24593, 49157, 98317, 196613, 393241, 786433, 1572869,
          3145739, 6291469, 12582917, 25165843, 50331653, 100663319, 201326611, 402653189, 805306457, 1610612741, 3221225473,
          4294967291]
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MSG_NO_EOF = "[bam_header_read] EOF marker is absent. The input is probably truncated.\n"
MSG_MAGIC = "[bam_header_read] invalid BAM binary header (this is not a BAM file).\n"
MSG_HEADER = "[bam_index_core] Invalid BAM header."
MSG_FAIL = "[bam_index_build2] fail to index the BAM file.\n"
MSG_UNPLACED_FIRST = "[bam_index_core] the alignment is not sorted: reads without coordinates prior to reads with coordinates.\n"


class Refuse(Exception):
    pass


class KhOrder:
    """The slots of an integer-keyed open-addressing table with prime bucket counts, double hashing and a resize at 0.77 load,
    keys never deleted: only WHERE every key lies matters, the index file lists a target's bins slot by slot."""

    def __init__(self):
        self.n = 0
        self.size = 0
        self.upper = 0
        self.keys = []
        self.used = []

    def _grow(self):
        want = self.n + 1
        t = len(PRIMES) - 1
        while PRIMES[t] > want:
            t -= 1
        new_n = PRIMES[t + 1]
        if self.size >= int(new_n * 0.77 + 0.5):
            return
        keys = self.keys + [0] * (new_n - self.n)
        old = list(self.used)              # True: holds a key that has not moved yet
        new_used = [False] * new_n
        for j in range(self.n):
            if not old[j]:
                continue
            key = keys[j]
            old[j] = False
            while True:                    # a key that lands on an unmoved one takes its slot and sends it on
                i = key % new_n
                inc = 1 + key % (new_n - 1)
                while new_used[i]:
                    i = i + inc - new_n if i + inc >= new_n else i + inc
                new_used[i] = True
                if i < self.n and old[i]:
                    keys[i], key = key, keys[i]
                    old[i] = False
                else:
                    keys[i] = key
                    break
        self.keys, self.used, self.n = keys, new_used, new_n
        self.upper = int(new_n * 0.77 + 0.5)

    def put(self, key):
        """True when the key is new"""
        if self.size >= self.upper:
            self._grow()
        i = key % self.n
        if self.used[i]:
            inc = 1 + key % (self.n - 1)
            while self.used[i] and self.keys[i] != key:
                i = i + inc - self.n if i + inc >= self.n else i + inc
        if self.used[i]:
            return False
        self.keys[i], self.used[i] = key, True
        self.size += 1
        return True

    def order(self):
        return [self.keys[i] for i in range(self.n) if self.used[i]]


class Bgzf:
    """bgzf_read over the file's bytes: which block is loaded, how far it is consumed, what bam_tell says"""

    def __init__(self, data):
        self.data = data
        self.at = 0                # the file position
        self.addr = 0
        self.block = b""
        self.off = 0

    def _load(self):
        addr = self.at
        h = self.data[self.at:self.at + 18]
        self.at += len(h)
        if not h:
            self.block = b""
            return 0
        if (len(h) != 18 or h[0] != 31 or h[1] != 139 or h[2] != 8 or not h[3] & 4 or h[10] | h[11] << 8 != 6 or h[12:14] != b"BC"
                or h[14] | h[15] << 8 != 2):
            return -1
        size = (h[16] | h[17] << 8) + 1
        rest = self.data[self.at:self.at + size - 18]
        self.at += len(rest)
        if len(rest) != size - 18:
            return -1
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress((h + rest)[18:18 + size - 16], 65536)
        except zlib.error:
            return -1
        if not d.eof:
            return -1
        if self.block:
            self.off = 0
        self.addr, self.block = addr, out
        return 0

    def read(self, n):
        """the bytes, or None after a failed block"""
        out = b""
        if n <= 0:
            return out
        while len(out) < n:
            avail = len(self.block) - self.off
            if avail <= 0:
                if self._load() != 0:
                    return None
                avail = len(self.block) - self.off
                if avail <= 0:
                    break
            k = min(n - len(out), avail)
            out += self.block[self.off:self.off + k]
            self.off += k
        if self.off == len(self.block):
            self.addr, self.off, self.block = self.at, 0, b""
        return out

    def tell(self):
        return self.addr << 16 | (self.off & 0xffff)


def calend(pos, cigar):
    """bam_calend as a 32-bit unsigned number: the position behind the record on the reference, `B` operations included"""
    end = pos
    for k, c in enumerate(cigar):
        op, ln = c & 15, c >> 4
        if op == 9:
            if k == len(cigar) - 1:
                break
            u = v = 0
            l = k - 1
            while l >= 0:
                op1, len1 = cigar[l] & 15, cigar[l] >> 4
                kind = 0x3C1A7 >> (op1 << 1) & 3
                if kind & 1:
                    if u + len1 >= ln:
                        if kind & 2:
                            v += ln - u
                        break
                    u += len1
                if kind & 2:
                    v += len1
                l -= 1
            end = pos if l < 0 else end - v
        elif 0x3C1A7 >> (op << 1) & 2:
            end += ln
    return end & 0xffffffff


def read1(z):
    """(status, record): status >= 0 with the record's fields, else bam_read1's negative code"""
    b = z.read(4)
    if b is None or len(b) != 4:
        return (-1 if b is not None and len(b) == 0 else -2), None
    (block_len,) = struct.unpack("<i", b)
    core = z.read(32)
    if core is None or len(core) != 32:
        return -3, None
    tid, pos, x2, x3 = struct.unpack_from("<iiII", core)
    want = block_len - 32
    data = z.read(want)
    if data is None or len(data) != want:      # (a size under 32 reads nothing and is short as well)
        return -4, None
    l_name, n_cigar = x2 & 0xff, x3 & 0xffff
    return 4 + block_len, dict(tid=tid, pos=pos, bin=x2 >> 16, flag=x3 >> 16, l_name=l_name, n_cigar=n_cigar, data=data)


def cigar_of(r):
    if r["l_name"] + 4 * r["n_cigar"] > len(r["data"]):
        raise Refuse("name and CIGAR do not fit the record")
    return struct.unpack_from("<%dI" % r["n_cigar"], r["data"], r["l_name"])


def name_of(r):
    d = r["data"]
    k = d.find(b"\0")
    if k < 0:
        raise Refuse("a read name without its end")
    return d[:k].decode("latin-1")


def s32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def index(data):
    err = ""
    z = Bgzf(data)
    if len(data) < 28 or data[-28:] != EOF_BLOCK:
        err += MSG_NO_EOF
    magic = z.read(4)
    if magic is None or magic != b"BAM\1":
        return None, err + MSG_MAGIC + MSG_HEADER + MSG_FAIL

    def need(n):
        b = z.read(n)
        if b is None or len(b) != n:
            raise Refuse("the header ends early")
        return b

    (l_text,) = struct.unpack("<i", need(4))
    if l_text < 0:
        raise Refuse("l_text")
    need(l_text)
    (n_ref,) = struct.unpack("<i", need(4))
    if n_ref < 0:
        raise Refuse("n_ref")
    for _ in range(n_ref):
        (l_name,) = struct.unpack("<i", need(4))
        if l_name < 0:
            raise Refuse("l_name")
        need(l_name + 4)

    tables = [KhOrder() for _ in range(n_ref)]
    lists = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    lin_n = [0] * n_ref

    def insert(tid, b, beg, end):
        if tables[tid].put(b):
            lists[tid][b] = []
        lists[tid][b].append([beg, end])

    NONE = 0xffffffff
    save_bin = last_bin = NONE
    save_tid = last_tid = -1
    last_coor = -1
    save_off = last_off = off_beg = off_end = z.tell()
    n_mapped = n_unmapped = n_no_coor = 0
    ret = 0
    while True:
        ret, r = read1(z)
        if ret < 0:
            break
        tid, pos = r["tid"], r["pos"]
        if tid < -1 or tid >= n_ref:
            raise Refuse("refID outside the header's targets")
        if tid < 0:
            n_no_coor += 1
        if last_tid < tid or (last_tid >= 0 and tid < 0):
            last_tid, last_bin = tid, NONE
        elif (last_tid & 0xffffffff) > (tid & 0xffffffff):
            return None, err + "[bam_index_core] the alignment is not sorted (%s): %d-th chr > %d-th chr\n" % (name_of(r), last_tid + 1, tid + 1) + MSG_FAIL
        elif tid >= 0 and last_coor > pos:
            return None, err + "[bam_index_core] the alignment is not sorted (%s): %d > %d in %d-th chr\n" % (
                name_of(r), last_coor & 0xffffffff, pos & 0xffffffff, tid + 1) + MSG_FAIL
        if tid >= 0 and not r["flag"] & 4:
            if pos < 0:
                raise Refuse("a mapped record with a negative position")
            beg = pos >> 14
            end = s32(((calend(pos, cigar_of(r)) - 1) & 0xffffffff) >> 14)
            for w in range(beg, end + 1):
                if lin[tid].get(w, 0) == 0:
                    lin[tid][w] = last_off
            lin_n[tid] = end + 1
        if r["bin"] != last_bin:
            if save_bin != NONE:
                insert(save_tid, save_bin, save_off, last_off)
            if last_bin == NONE and save_tid != -1:
                off_end = last_off
                insert(save_tid, META_BIN, off_beg, off_end)
                insert(save_tid, META_BIN, n_mapped, n_unmapped)
                n_mapped = n_unmapped = 0
                off_beg = off_end
            save_off = last_off
            save_bin = last_bin = r["bin"]
            save_tid = tid
            if save_tid < 0:
                break
        if z.tell() <= last_off:
            return None, err + "[bam_index_core] bug in BGZF/RAZF: %x < %x\n" % (z.tell(), last_off) + MSG_FAIL
        if r["flag"] & 4:
            n_unmapped += 1
        else:
            n_mapped += 1
        last_off = z.tell()
        last_coor = pos
    if save_tid >= 0:
        insert(save_tid, save_bin, save_off, z.tell())
        insert(save_tid, META_BIN, off_beg, z.tell())
        insert(save_tid, META_BIN, n_mapped, n_unmapped)
    for t in range(n_ref):
        for b, ch in lists[t].items():
            if b == META_BIN:
                continue
            kept = [ch[0]]
            for c in ch[1:]:
                if kept[-1][1] >> 16 == c[0] >> 16:
                    kept[-1][1] = c[1]
                else:
                    kept.append(c)
            lists[t][b] = kept
    if ret >= 0:
        while True:
            ret, r = read1(z)
            if ret < 0:
                break
            n_no_coor += 1
            if r["tid"] >= 0:
                return None, err + MSG_UNPLACED_FIRST + MSG_FAIL
    if ret < -1:
        err += "[bam_index_core] truncated file? Continue anyway. (%d)\n" % ret
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for t in range(n_ref):
        order = tables[t].order()
        out.append(struct.pack("<i", len(order)))
        for b in order:
            ch = lists[t][b]
            out.append(struct.pack("<Ii", b, len(ch)))
            out += [struct.pack("<QQ", c[0], c[1]) for c in ch]
        out.append(struct.pack("<i", lin_n[t]))
        prev = 0
        vals = []
        for w in range(lin_n[t]):
            v = lin[t].get(w, 0)
            if v == 0 and w > 0:
                v = prev
            prev = v
            vals.append(v)
        out.append(struct.pack("<%dQ" % len(vals), *vals))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out), err
