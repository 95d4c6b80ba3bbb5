"""A DEFLATE stream builder written from RFC 1951, for streams zlib's deflate never writes.

Nothing here knows the decoders under test.  The caller dictates everything an encoder normally chooses: the code lengths
(no optimisation step: canonical codes straight from the list), how the code lengths are run-length coded (separately for
the two alphabets as zlib does, or as one array as libdeflate does, or symbol by symbol), HLIT / HDIST / HCLEN, which of two
spellings a length gets, the bit phase a stored block starts at.  zlib's INFLATE accepts all of RFC 1951 and is the oracle:
tests/test_deflate_craft_host.py holds every stream of tests/deflate_cases.py to it before any decoder sees one.

Tokens of a block: an int 0..255 is a literal; (length, dist) a match; (length, dist, lensym) a match whose length is spelled
with that length symbol; ("L", sym, extra, nbits) / ("D", sym, extra, nbits) a raw literal/length / distance symbol with its
extra bits; ("bits", value, n) raw bits.  The end-of-block code is appended by the block writers unless eob=False.
"""
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """LSB-first, as RFC 1951 3.1.1 packs everything but the Huffman codes themselves (code(): MSB-first)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return len(self.out) * 8 + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        r = 0
        for _ in range(n):
            r = r << 1 | (code & 1)
            code >>= 1
        self.bits(r, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """[(code, nbits)] per symbol (RFC 1951 3.2.2), whatever the lengths: an over-subscribed list gets the codes the
    algorithm gives it, truncated to their length."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append((0, 0))
    return out


def kraft(lengths, unit=15):
    return sum(1 << (unit - l) for l in lengths if l)


def len_symbol(length):
    if length == 258:
        return 285
    k = 0
    while k + 1 < 28 and LEN_BASE[k + 1] <= length:
        k += 1
    return 257 + k


def dist_symbol(dist):
    k = 0
    while k + 1 < 30 and DIST_BASE[k + 1] <= dist:
        k += 1
    return k


def symbols_of(tokens):
    """The (literal/length, distance) symbols a token list uses, for building a code that covers it."""
    lit, dst = [], []
    for t in tokens:
        if isinstance(t, int):
            lit.append(t)
        elif t[0] == "L":
            lit.append(t[1])
        elif t[0] == "D":
            dst.append(t[1])
        elif t[0] == "bits":
            pass
        else:
            lit.append(t[2] if len(t) > 2 else len_symbol(t[0]))
            dst.append(dist_symbol(t[1]))
    return lit, dst


def put_tokens(w, tokens, lit_lens, dist_lens):
    lc, dc = canonical(lit_lens), canonical(dist_lens)

    def lit(sym):
        assert lc[sym][1], ("literal/length symbol without a code", sym)
        w.code(*lc[sym])

    def dst(sym):
        assert dc[sym][1], ("distance symbol without a code", sym)
        w.code(*dc[sym])

    for t in tokens:
        if isinstance(t, int):
            lit(t)
        elif t[0] == "L":
            lit(t[1])
            w.bits(t[2], t[3])
        elif t[0] == "D":
            dst(t[1])
            w.bits(t[2], t[3])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        else:
            length, dist = t[0], t[1]
            ls = t[2] if len(t) > 2 else len_symbol(length)
            k = ls - 257
            assert 0 <= length - LEN_BASE[k] < (1 << LEN_EXTRA[k]) or (LEN_EXTRA[k] == 0 and length == LEN_BASE[k]), t
            lit(ls)
            w.bits(length - LEN_BASE[k], LEN_EXTRA[k])
            ds = dist_symbol(dist)
            dst(ds)
            w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])


def expand(tokens, history=b""):
    """What a token list decodes to (matches only): the builder's own statement of the intended bytes."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            if t < 256:
                out.append(t)
        elif t[0] in ("L", "D", "bits"):
            raise ValueError("raw tokens have no intended bytes")
        else:
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out), t
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(history):])


# ---- block writers -----------------------------------------------------------------------------------------------------------
def stored_block(w, data, final=False, nlen=None, length=None):
    """Stored block (3.2.4) from whatever bit phase the writer is at.  length / nlen: the header fields, if not the true ones."""
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    n = len(data) if length is None else length
    w.bits(n, 16)
    w.bits((n ^ 0xffff) if nlen is None else nlen, 16)
    w.raw(data)


def fixed_block(w, tokens, final=False, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, list(tokens) + ([256] if eob else []), FIXED_LIT, FIXED_DIST)


def rle_lengths(lens):
    """Greedy run-length coding of one array of code lengths -> [(symbol, extra value)]."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        j = i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def flat_complete(freq, n_syms=19):
    """A COMPLETE code over the used symbols with two neighbouring lengths, the frequent ones shorter (no Huffman step: the
    code-length code only has to be valid)."""
    used = sorted((s for s in range(n_syms) if freq.get(s, 0)), key=lambda s: (-freq[s], s))
    if len(used) == 1:
        used.append(0 if used[0] != 0 else 1)           # zlib refuses an incomplete code-length code
    k = 1
    while (1 << k) < len(used):
        k += 1
    short = (1 << k) - len(used)
    lens = [0] * n_syms
    for r, s in enumerate(used):
        lens[s] = k - 1 if r < short else k
    return lens


def dynamic_block(w, lit_lens, dist_lens, tokens, final=False, rle="zlib", hclen19=False, cl_lens=None, eob=True,
                  hlit_field=None, hdist_field=None):
    """Dynamic block (3.2.7).  len(lit_lens) is HLIT (257..286 in a valid block), len(dist_lens) HDIST (1..30).
    rle: "none" | "zlib" (two sequences) | "joint" (one) | a list of (symbol, extra value) pairs written as given.
    cl_lens: the 19 code-length-code lengths, if the caller dictates them too."""
    both = list(lit_lens) + list(dist_lens)
    if rle == "none":
        seq = [(l, 0) for l in both]
    elif rle == "zlib":
        seq = rle_lengths(list(lit_lens)) + rle_lengths(list(dist_lens))
    elif rle == "joint":
        seq = rle_lengths(both)
    else:
        seq = list(rle)
    if cl_lens is None:
        freq = {}
        for s, _ in seq:
            freq[s] = freq.get(s, 0) + 1
        cl_lens = flat_complete(freq)
    hclen = 19
    if not hclen19:
        while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit_field is None else hlit_field, 5)
    w.bits(len(dist_lens) - 1 if hdist_field is None else hdist_field, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cc = canonical(cl_lens)
    for s, x in seq:
        assert cc[s][1], ("code-length symbol without a code", s)
        w.code(*cc[s])
        if s >= 16:
            w.bits(x, CL_EXTRA[s])
    put_tokens(w, list(tokens) + ([256] if eob else []), lit_lens, dist_lens)


# ---- an encoder "as another encoder would" -----------------------------------------------------------------------------------
def lz77_tokens(data, chain=4, min_len=3, max_len=258, window=32768):
    """Greedy LZ77 (hash of 3 bytes, bounded chain).  The ratio does not matter; the matches are real ones."""
    n = len(data)
    head, prev = {}, [0] * n
    out, i = [], 0
    while i < n:
        best_l, best_d = 0, 0
        if i + min_len <= n:
            key = data[i:i + 3]
            c = head.get(key, -1)
            tries = chain
            while c >= 0 and tries and i - c <= window:
                l, lim = 0, min(max_len, n - i)
                while l < lim and data[c + l] == data[i + l]:
                    l += 1
                if l > best_l:
                    best_l, best_d = l, i - c
                    if l == lim:
                        break
                c = prev[c] - 1
                tries -= 1
        step = best_l if best_l >= min_len else 1
        out.append((best_l, best_d) if best_l >= min_len else data[i])
        for j in range(i, min(i + step, n - 2)):
            key = data[j:j + 3]
            prev[j] = head.get(key, -1) + 1
            head[key] = j
        i += step
    return out


def limited_lengths(freq, n_syms, limit=15):
    """Huffman code lengths of the used symbols, held to `limit` bits by halving the frequencies until they fit (a simple
    length-limiting rule; optimality is not the point)."""
    f = {s: c for s, c in freq.items() if c}
    while True:
        lens = [0] * n_syms
        if len(f) == 1:
            lens[next(iter(f))] = 1
            return lens
        heap = [(c, s, None, None) for s, c in f.items()]
        heapq.heapify(heap)
        tick = n_syms
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            heapq.heappush(heap, (a[0] + b[0], tick, a, b))
            tick += 1
        stack = [(heap[0], 0)]
        while stack:
            node, d = stack.pop()
            if node[2] is None:
                lens[node[1]] = d
            else:
                stack += [(node[2], d + 1), (node[3], d + 1)]
        if max(lens) <= limit:
            return lens
        f = {s: max(1, c >> 1) for s, c in f.items()}


def trim_tail(lens, least):
    lens = list(lens)
    while len(lens) > least and lens[-1] == 0:
        lens.pop()
    return lens


def encode_block(w, tokens, final=False, rle="joint", limit=15):
    """One dynamic block whose codes come from the tokens' own frequencies."""
    lit, dst = symbols_of(tokens)
    fl, fd = {256: 1}, {}
    for s in lit:
        fl[s] = fl.get(s, 0) + 1
    for s in dst:
        fd[s] = fd.get(s, 0) + 1
    ll = trim_tail(limited_lengths(fl, 286, limit), 257)
    dl = trim_tail(limited_lengths(fd, 30, limit), 1) if fd else [0]
    dynamic_block(w, ll, dl, tokens, final, rle)


def encode_stream(data, block_symbols, rle="joint", chain=4, final=True, tokens=None):
    """`data` as a sequence of dynamic blocks of block_symbols[k % len] tokens each -> (bytes, [bit position of every block])."""
    tokens = lz77_tokens(data, chain) if tokens is None else tokens
    w, starts, i, k = BitWriter(), [], 0, 0
    while True:
        n = block_symbols[k % len(block_symbols)]
        starts.append(w.bitpos)
        last = i + n >= len(tokens)
        encode_block(w, tokens[i:i + n], final and last, rle)
        i += n
        k += 1
        if last:
            break
    if not final:
        stored_block(w, b"")                              # (a sync marker: the stream ends on a byte)
    return w.getvalue(), starts


# ---- table room --------------------------------------------------------------------------------------------------------------
def table_need(lengths, root):
    """Entries a two-level decoding table takes for this code: 2^root, plus one sub-table per root prefix that has longer
    codes under it, as wide as the LONGEST code under that prefix."""
    codes = canonical(lengths)
    longest = {}
    for (c, l) in codes:
        if l > root:
            p = c >> (l - root)
            longest[p] = max(longest.get(p, 0), l)
    return (1 << root) + sum(1 << (l - root) for l in longest.values())


def lengths_from_counts(counts):
    """{length: how many} -> a list of lengths, shortest first."""
    return [l for l in sorted(counts) for _ in range(counts[l])]


LIT_852 = {1: 1, 2: 1, 3: 1, 10: 45, 11: 137, 12: 17, 13: 81, 14: 1, 15: 2}
DIST_400 = {2: 3, 3: 1, 4: 1, 5: 1, 9: 13, 10: 5, 11: 1, 12: 1, 13: 1, 14: 1, 15: 2}


def _count_vectors(l, l_to, left, rem, max_len, acc):
    """Every (counts of lengths l .. l_to, open slots behind them, symbols left) that a complete code of lengths up to max_len
    can still grow from: `left` slots of length l - 1 are open, `rem` symbols have no length yet."""
    if l > l_to:
        yield list(acc), left, rem
        return
    slots = 2 * left
    for c in range(0, min(slots, rem) + 1):
        rest, more = slots - c, rem - c
        if (rest == 0) != (more == 0):
            continue                                        # complete exactly when the symbols are used up
        # every later symbol fills at most half a slot of this length, and at least 2^-(max_len - l) of one
        if rest and (l == max_len or more < 2 * rest or more > rest << (max_len - l)):
            continue
        acc.append(c)
        yield from _count_vectors(l + 1, l_to, rest, more, max_len, acc)
        acc.pop()


def worst_table_need(n_syms, root, max_len=15):
    """The largest table_need over ALL complete codes of n_syms symbols with lengths up to max_len.  Every distribution of the
    lengths up to `root` is walked; what the longer codes add depends on it only through how many root prefixes stay open and
    how many symbols are left, so the distributions of the longer lengths are enumerated (all of them) once per such pair."""
    best, worst = {}, 0
    for head, left, rem in _count_vectors(1, root, 1, n_syms, max_len, []):
        if (left, rem) not in best:
            best[left, rem] = max((table_need([l for l, c in enumerate(head + tail, 1) for _ in range(c)], root)
                                   for tail, _, _ in _count_vectors(root + 1, max_len, left, rem, max_len, [])), default=0)
        worst = max(worst, best[left, rem])
    return worst


# ---- containers --------------------------------------------------------------------------------------------------------------
def gzip_member(deflate, payload, name=None):
    head = bytes([0x1f, 0x8b, 8, 8 if name else 0, 0, 0, 0, 0, 0, 3]) + ((name + b"\0") if name else b"")
    return head + deflate + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload) & 0xffffffff)


def bgzf_block(deflate, payload):
    assert len(payload) <= 65536 and len(deflate) + 26 <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(deflate) + 25) + deflate +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_file(data, block_bytes, block_symbols=(3000, 700, 9000), rle="joint"):
    out = b""
    for a in range(0, len(data), block_bytes):
        piece = data[a:a + block_bytes]
        out += bgzf_block(encode_stream(piece, block_symbols, rle)[0], piece)
    return out + BGZF_EOF


def zlib_inflate(stream):
    """-> the bytes, or None where zlib refuses the stream or calls it unfinished."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None
    return out if d.eof else None
