"""The crafted DEFLATE streams of tests/test_deflate_craft_host.py and tests/test_inflate_foreign_gpu.py: what RFC 1951 allows
and zlib's deflate never writes (accept_cases) and what it forbids (reject_cases), built with tests/deflate_craft.py.

A case is written by a function fn(w, final): it appends whole blocks to the bit writer, the last of them with BFINAL = final,
and returns the bytes the blocks stand for.  Case.stream is the form with a final block; Case.open_stream the one without,
ended by an empty stored block so that it ends on a byte like a sync flush -- the form that can sit between two zlib-written
stretches of one stream."""
import os
import struct
import zlib

import numpy as np

import deflate_craft as dc
from deflate_craft import BitWriter, dynamic_block, fixed_block, stored_block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
    def __init__(self, name, fn):
        self.name, self.fn = name, fn
        w = BitWriter()
        self.want = fn(w, True)
        self.stream = w.getvalue()
        w = BitWriter()
        assert fn(w, False) == self.want
        stored_block(w, b"")
        self.open_stream = w.getvalue()

    def __repr__(self):
        return self.name


def complete(lens, fill):
    """Give unused symbols of `fill` the lengths that make the code complete (one symbol per set bit of what is missing)."""
    lens = list(lens)
    rem = 32768 - dc.kraft(lens)
    assert 0 <= rem < 32768, rem
    fill = [s for s in fill if lens[s] == 0]
    for b in range(14, -1, -1):
        if rem >> b & 1:
            lens[fill.pop(0)] = 15 - b
    assert dc.kraft(lens) == 32768
    return lens


def exercise(lit_lens, dist_lens, written, rng, rounds=2, start=()):
    """Tokens that use every symbol the two codes have (every distance symbol whose distances are in reach), at the lowest,
    the highest and random extra-bits values -> (tokens, units of output they make)."""
    lits = [s for s in range(min(256, len(lit_lens))) if lit_lens[s]]
    lens = [s for s in range(257, len(lit_lens)) if lit_lens[s]]
    dsts = [s for s in range(len(dist_lens)) if dist_lens[s]]
    toks, n = list(start), written + len(start)
    for r in range(rounds):
        for s in lits:
            toks.append(s)
            n += 1
        k = 0
        for ls in (lens if dsts else []):
            for pick in range(3):
                ds = dsts[(k + r) % len(dsts)]
                k += 1
                if dc.DIST_BASE[ds] > n:
                    ds = max(d for d in dsts if dc.DIST_BASE[d] <= n) if any(dc.DIST_BASE[d] <= n for d in dsts) else None
                if ds is None:
                    continue
                span_l, span_d = (1 << dc.LEN_EXTRA[ls - 257]) - 1, (1 << dc.DIST_EXTRA[ds]) - 1
                xl = (0, span_l, int(rng.integers(0, span_l + 1)))[pick]
                xd = (0, span_d, int(rng.integers(0, span_d + 1)))[(pick + r) % 3]
                dist = min(dc.DIST_BASE[ds] + xd, n)
                length = dc.LEN_BASE[ls - 257] + xl if ls != 285 else 258
                toks.append((length, dist, ls))
                n += length
    return toks, n - written


def history(w, rng, n=32768):
    """A stored block of random bytes in front: what far distances reach into."""
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    stored_block(w, data)
    return data


# ---- 1. code-length runs across the literal/distance boundary ---------------------------------------------------------------
def _boundary(sym, rep, k):
    """One run symbol `sym` (16 / 17 / 18) of `rep` entries that starts k entries in front of the boundary between the HLIT
    literal/length lengths and the HDIST distance lengths; every other length is sent by itself.  A 16 repeats the value 6,
    so both codes' Kraft sums move; both codes are then completed with symbols outside the run."""
    hlit, hdist = 286, 30
    a = hlit - k
    b = a + rep
    assert 257 <= a and b <= hlit + hdist - 1
    v = 6 if sym == 16 else 0
    held = set(range(a - (1 if sym == 16 else 0), b))      # (a 16 repeats the entry in front of it)
    joint = [v if i in held else 0 for i in range(hlit + hdist)]
    lit, dst = joint[:hlit], joint[hlit:]
    lit[256] = 3
    lit = complete(lit, [s for s in list(range(97, 123)) + list(range(257, 262)) if s not in held])
    dst[29] = 2
    dst = complete(dst, [s for s in range(28, -1, -1) if s + hlit not in held])
    both = lit + dst
    assert all(both[i] == v for i in held)
    seq = [(l, 0) for l in both[:a]] + [(sym, rep - {16: 3, 17: 3, 18: 11}[sym])] + [(l, 0) for l in both[b:]]

    def fn(w, final):
        rng = np.random.default_rng(1000 * sym + 10 * rep + k)
        hist = history(w, rng)
        toks, _ = exercise(lit, dst, len(hist), rng)
        dynamic_block(w, lit, dst, toks, final, rle=seq)
        return hist + dc.expand(toks, hist)
    return Case("run%d_rep%d_starts%d_before" % (sym, rep, k), fn)

def _run18_to_the_end():
    """One 18 run that zeroes the tail of the literal/length lengths and the whole distance array."""
    hlit, hdist = 280, 7
    lit = [0] * hlit
    lit[256] = 2
    lit = complete(lit, range(65, 91))
    a = 257
    seq = [(l, 0) for l in lit[:a]] + [(18, hlit + hdist - a - 11)]

    def fn(w, final):
        toks = [s for s in range(256) if lit[s]] * 9
        dynamic_block(w, lit, [0] * hdist, toks, final, rle=seq)
        return bytes(toks)
    return Case("run18_zeroes_tail_and_all_distances", fn)


# ---- 2. header extremes ------------------------------------------------------------------------------------------------------
def _hclen_shortest():
    """HLIT 257, HDIST 1, and the shortest HCLEN a valid block can have: 5 (16 17 18 0 8) -- with the first four alone every
    length would be 0 and there would be no end-of-block code.  255 literals and the end-of-block code, all of 8 bits."""
    lit = [8] * 255 + [0, 8]

    def fn(w, final):
        toks = list(range(255)) + [254, 0, 17]
        cl = [0] * 19
        cl[0] = cl[8] = 1
        dynamic_block(w, lit, [0], toks, final, rle="none", cl_lens=cl)
        return bytes(toks)
    return Case("hlit257_hdist1_hclen5", fn)


def _hclen_field4():
    """HCLEN field 4: eight code-length-code lengths (16 17 18 0 8 7 9 6), and no more symbols than those to write with."""
    lit = [0] * 257
    lit[256] = 6
    for s in range(31):
        lit[48 + s] = 6                                    # 32 codes of 6 bits: 1/2
    for s in range(32):
        lit[97 + s] = 7                                    # 32 of 7: 1/4
    for s in range(64):
        lit[160 + s] = 8                                   # 64 of 8: 1/4
    assert dc.kraft(lit) == 32768
    cl = [0] * 19
    cl[16], cl[18], cl[0], cl[6], cl[7], cl[8] = 2, 2, 3, 3, 3, 3

    def fn(w, final):
        toks = [s for s in range(256) if lit[s]] + [50, 100, 200]
        at = w.bitpos
        dynamic_block(w, lit, [0], toks, final, rle="zlib", cl_lens=cl)
        assert (w.getvalue()[at // 8] | w.getvalue()[at // 8 + 1] << 8 | w.getvalue()[at // 8 + 2] << 16) >> (at % 8 + 13) & 15 == 4
        return bytes(toks)
    return Case("hclen_field4", fn)

def _cl_length7():
    """A code-length code with lengths 1 .. 7, 7: eight symbols, the values 0 .. 7 of a literal code 1 2 3 4 5 6 7 7."""
    lit = [0] * 258
    for s, l in zip(b"gabcde", (1, 2, 3, 4, 5, 6)):
        lit[s] = l
    lit[256] = lit[257] = 7
    dst = [1, 1]
    cl = [0] * 19
    for s, l in ((0, 1), (7, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (6, 7)):
        cl[s] = l

    def fn(w, final):
        toks = list(b"gabcdegg") + [(3, 1), (3, 2), (3, 2)] + list(b"edc")
        dynamic_block(w, lit, dst, toks, final, rle="none", cl_lens=cl)
        return dc.expand(toks)
    return Case("code_length_code_of_7_bits", fn)

# ---- 3. empty and single-symbol codes ---------------------------------------------------------------------------------------
def _no_distance_code():
    lit = [0] * 257
    lit[256] = 3
    lit = complete(lit, range(65, 91))

    def fn(w, final):
        toks = [s for s in range(256) if lit[s]] * 40
        dynamic_block(w, lit, [0], toks, final, rle="joint")
        return bytes(toks)
    return Case("no_distance_code", fn)


def _one_distance_code(at):
    """ONE distance code, of length 1 (half of the code space stays empty): distance symbol `at`, used by matches."""
    lit = [0] * 270
    lit[256] = lit[257] = 4
    lit[258] = lit[264] = lit[269] = 3
    lit[65] = 1
    assert dc.kraft(lit) == 32768
    dst = [0] * at + [1]

    def fn(w, final):
        rng = np.random.default_rng(30 + at)
        toks, _ = exercise(lit, dst, 0, rng, start=[65] * 8)
        dynamic_block(w, lit, dst, toks, final, rle="joint")
        return dc.expand(toks)
    return Case("one_distance_code_symbol%d" % at, fn)

def _only_end_of_block():
    def fn(w, final):
        for k in range(3):
            dynamic_block(w, [0] * 256 + [1], [0], [], False, rle="joint")
        toks = list(b"after blocks that hold nothing but their end")
        fixed_block(w, toks, False)
        dynamic_block(w, [0] * 256 + [1], [0], [], final, rle="zlib")
        return bytes(toks)
    return Case("only_an_end_of_block_code", fn)


# ---- 4. the widest symbols ---------------------------------------------------------------------------------------------------
def _wide_codes():
    lit = [0] * 286
    for s, l in ((65, 1), (256, 2), (66, 3), (67, 4), (68, 5), (284, 15), (120, 15), (121, 15), (122, 15)):
        lit[s] = l
    lit = complete(lit, range(97, 120))
    dst = [0] * 30
    dst[28] = dst[29] = 15
    dst = complete(dst, range(0, 28))
    return lit, dst


def _wide_at_every_offset():
    """Length symbol 284 (15 + 5 bits) and distance symbol 29 (15 + 13 bits): the 48-bit match at every bit offset of the
    block's first 64 bits, behind 0 .. 63 one-bit literals; then 15-bit literals."""
    lit, dst = _wide_codes()

    def fn(w, final):
        rng = np.random.default_rng(44)
        out = bytearray(history(w, rng))
        for f in range(64):
            toks = [65] * f + [(227 + int(rng.integers(0, 31)), 24577 + int(rng.integers(0, 8192)), 284), 120, 121, 122, 66]
            toks += [(227 + f % 31, 32768 - f, 284)]
            dynamic_block(w, lit, dst, toks, final and f == 63, rle="joint")
            out += dc.expand(toks, bytes(out[-32768:]))
        return bytes(out)
    return Case("widest_match_at_every_window_offset", fn)


def _wide_across_refills(phase):
    """The same 48-bit match across every 256-byte boundary of the compressed stream in the 2 KiB behind the block's start,
    with 1 .. 47 of its bits in front of the boundary."""
    lit, dst = _wide_codes()

    def fn(w, final):
        rng = np.random.default_rng(45 + phase)
        hist = history(w, rng, 32768 - 5 * phase)          # (the stored bytes move the block's own start, too)
        dynamic_block(w, lit, dst, [], False, rle="joint", eob=False)
        toks = []
        cuts = [1, 8, 17, 24, 31, 40, 47, 33, 2, 46]
        for j in range(8):
            boundary = (w.bitpos // 2048 + 1) * 2048
            lead = cuts[(j + phase) % len(cuts)]
            assert boundary - lead - w.bitpos >= 0
            part = [65] * (boundary - lead - w.bitpos) + [(227 + int(rng.integers(0, 31)), 24577 + int(rng.integers(0, 8000)), 284), 122]
            dc.put_tokens(w, part, lit, dst)
            toks += part
        dc.put_tokens(w, [256], lit, dst)
        fixed_block(w, [10], final)
        return hist + dc.expand(toks, hist) + b"\n"
    return Case("widest_match_across_ring_refills_%d" % phase, fn)


# ---- 5. table room -----------------------------------------------------------------------------------------------------------
def _table_room(reverse):
    lit = dc.lengths_from_counts(dc.LIT_852)
    dst = dc.lengths_from_counts(dc.DIST_400)
    if reverse:
        lit, dst = lit[::-1], dst[::-1]

    def fn(w, final):
        rng = np.random.default_rng(50 + reverse)
        hist = history(w, rng)
        toks, _ = exercise(lit, dst, len(hist), rng, rounds=2)
        dynamic_block(w, lit, dst, toks, final, rle="joint", hclen19=True)
        return hist + dc.expand(toks, hist)
    return Case("table_room_852_and_400" + ("_reversed" if reverse else ""), fn)


# ---- 6. dense windows and nested literal pairs -------------------------------------------------------------------------------
def _one_bit_literals():
    lit = [0] * 257
    lit[65] = lit[256] = 1

    def fn(w, final):
        dynamic_block(w, lit, [0], [65] * 5000, final, rle="joint")
        return b"A" * 5000
    return Case("one_bit_literals", fn)


def _nested_pairs():
    lit = [0] * 257
    lit[65], lit[66], lit[67], lit[256] = 1, 2, 3, 3

    def fn(w, final):
        rng = np.random.default_rng(61)
        toks = [int(x) for x in rng.choice([65, 66, 67], 3000, p=[0.5, 0.3, 0.2])]
        dynamic_block(w, lit, [0], toks, final, rle="joint")
        return bytes(toks)
    return Case("nested_literal_pairs", fn)


# ---- 7. length spellings -----------------------------------------------------------------------------------------------------
def _length_258_both_ways():
    def fn(w, final):
        toks = list(b"xyz") + [(258, 3), (258, 3, 284), (258, 1, 284), (258, 1), 33, (258, 2, 284), (258, 5)]
        fixed_block(w, toks, False)
        dc.encode_block(w, toks, final, rle="joint")
        return dc.expand(toks) + dc.expand(toks, dc.expand(toks))
    return Case("length_258_as_285_and_as_284_plus_31", fn)


def _every_length_and_distance(dynamic):
    def fn(w, final):
        rng = np.random.default_rng(71)
        hist = history(w, rng)
        ds = [d for s in range(30) for d in (dc.DIST_BASE[s], dc.DIST_BASE[s] + (1 << dc.DIST_EXTRA[s]) - 1)]
        toks = [(3 + k % 256, ds[k % len(ds)]) for k in range(2 * 256 + 60)]
        if dynamic:
            dc.encode_block(w, toks, final, rle="joint")
        else:
            fixed_block(w, toks, final)
        return hist + dc.expand(toks, hist)
    return Case("every_length_and_distance_code_" + ("dynamic" if dynamic else "fixed"), fn)


def _distance_equals_written():
    def fn(w, final):
        toks, n = list(b"abc"), 3
        while n < 3000:
            length = min(n, 258) if n % 2 else min(n, 200)
            toks.append((length, n))
            n += length
            toks.append(48 + n % 10)
            n += 1
        fixed_block(w, toks, final)
        return dc.expand(toks)
    return Case("distance_equals_bytes_written", fn)


def _short_distance_runs():
    def fn(w, final):
        toks = [97, (258, 1), (258, 1), 98, 99, (258, 2), (258, 2), 100, 101, 102, (258, 3), (258, 3), (258, 1), (258, 2), (258, 3)]
        dc.encode_block(w, toks, False, rle="zlib")
        fixed_block(w, toks, final)
        a = dc.expand(toks)
        return a + dc.expand(toks, a)
    return Case("runs_of_258_at_distance_1_2_3", fn)


# ---- 8. stored blocks and trains of tiny blocks ------------------------------------------------------------------------------
def _stored_phases(length):
    """A stored block of LEN `length` behind a fixed block of p = 0 .. 7 nine-bit literals: its header starts at every bit phase."""
    def one(p):
        def fn(w, final):
            rng = np.random.default_rng(80 + p)
            data = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
            fixed_block(w, [200] * p, False)
            assert w.bitpos % 8 == (2 + p) % 8
            stored_block(w, data, final)
            return bytes([200] * p) + data
        return Case("stored_len%d_phase%d" % (length, (2 + p) % 8), fn)
    return [one(p) for p in range(8)]


def _stored_short_all_phases():
    def fn(w, final):
        out = b""
        todo = [(length, p) for length in (0, 1, 0) for p in range(8)]
        for k, (length, p) in enumerate(todo):
            fixed_block(w, [200 + p] * p, False)
            data = bytes([33 + p] * length)
            stored_block(w, data, final and k + 1 == len(todo))
            out += bytes([200 + p] * p) + data
        return out
    return Case("stored_len0_len1_every_phase", fn)

def _empty_fixed_blocks():
    def fn(w, final):
        for k in range(300):
            fixed_block(w, [], False)
        fixed_block(w, list(b"behind 300 empty blocks"), False)
        for k in range(7):
            fixed_block(w, [], final and k == 6)
        return b"behind 300 empty blocks"
    return Case("300_empty_fixed_blocks", fn)


def _one_literal_blocks():
    def fn(w, final):
        out = bytearray()
        for k in range(200):
            lit = [0] * 257
            c = 32 + k % 90
            lit[c] = lit[256] = 1
            dynamic_block(w, lit, [0], [c], final and k == 199, rle=("joint", "zlib", "none")[k % 3])
            out.append(c)
        return bytes(out)
    return Case("200_one_literal_dynamic_blocks", fn)


# ---- 9. payloads as another encoder would write them -------------------------------------------------------------------------
_memo = {}


def fastq_text():
    if "fq" not in _memo:
        with open(os.path.join(GOLDEN, "fastq", "syn_var_a.fq"), "rb") as f:
            _memo["fq"] = f.read()
    return _memo["fq"]


def fastq_tokens():
    if "fqtok" not in _memo:
        _memo["fqtok"] = dc.lz77_tokens(fastq_text(), chain=3)
    return _memo["fqtok"]


def bam_payloads():
    """The decompressed bytes of tests/golden/bam/e.bam, BGZF block by BGZF block."""
    with open(os.path.join(GOLDEN, "bam", "e.bam"), "rb") as f:
        raw = f.read()
    out, o = [], 0
    while o < len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append(zlib.decompress(raw[o + 12 + xlen:o + bsize - 8], -15))
        o += bsize
    return out


def _fastq_one_long_block():
    def fn(w, final):
        toks = fastq_tokens()[:60000]
        dc.encode_block(w, toks, final, rle="joint")
        return dc.expand(toks)
    return Case("fastq_one_block_of_60000_symbols", fn)


def _bam_block(k, data):
    def fn(w, final):
        if data:
            toks = dc.lz77_tokens(data, chain=8)
            half = len(toks) // 2
            dc.encode_block(w, toks[:half], False, rle="joint")
            dc.encode_block(w, toks[half:], final, rle="joint")
        else:
            fixed_block(w, [], final)
        return data
    return Case("bam_block_%d_reencoded" % k, fn)


class _ForeignZlib:
    """What bamio.repack_bam calls zlib, with the builder as its deflate."""
    DEFLATED = zlib.DEFLATED
    crc32 = staticmethod(zlib.crc32)

    class _Co:
        def compress(self, piece):
            stream, _ = dc.encode_stream(piece, (900, 150, 4000), rle="joint", chain=2)
            assert dc.zlib_inflate(stream) == piece
            return stream

        def flush(self):
            return b""

    @staticmethod
    def compressobj(*args):
        return _ForeignZlib._Co()


def repack_bam_foreign(src, dst, block):
    """bamio.repack_bam (the records in BGZF blocks of `block` bytes, + the index) with every block's DEFLATE stream written by
    the builder: joint code-length runs, dynamic blocks of 900 / 150 / 4000 symbols."""
    from highperformancengs_amd import bamio
    real = bamio.zlib
    bamio.zlib = _ForeignZlib
    try:
        return bamio.repack_bam(src, dst, block)
    finally:
        bamio.zlib = real


def accept_cases():
    if "accept" in _memo:
        return _memo["accept"]
    cases = []
    # (an 18 run of more than 29 entries cannot cross the boundary and leave a distance code: 25 and 11 it is)
    for sym, rep in ((16, 6), (16, 3), (17, 10), (17, 3), (18, 25), (18, 11)):
        for k in sorted({1, 2, rep - 1, rep, 0}):         # rep: ends exactly on the boundary; 0: starts exactly on it
            cases.append(_boundary(sym, rep, k))
    cases.append(_run18_to_the_end())
    cases += [_hclen_shortest(), _hclen_field4(), _cl_length7()]
    cases += [_no_distance_code(), _one_distance_code(0), _one_distance_code(5), _only_end_of_block()]
    cases += [_wide_at_every_offset(), _wide_across_refills(0), _wide_across_refills(1), _wide_across_refills(2)]
    cases += [_table_room(False), _table_room(True)]
    cases += [_one_bit_literals(), _nested_pairs()]
    cases += [_length_258_both_ways(), _every_length_and_distance(False), _every_length_and_distance(True), _distance_equals_written(),
              _short_distance_runs()]
    cases += [_stored_short_all_phases()] + _stored_phases(65535) + [_empty_fixed_blocks(), _one_literal_blocks()]
    cases += [_fastq_one_long_block()] + [_bam_block(k, d) for k, d in enumerate(bam_payloads())]
    assert len({c.name for c in cases}) == len(cases)
    _memo["accept"] = cases
    return cases


# ---- what RFC 1951 forbids ---------------------------------------------------------------------------------------------------
class Reject:
    """A case is written by fn(w, final), the bad block carrying BFINAL = final.  stream: refused by zlib as it stands.
    open_stream (where the case has one): the bad block is not a final one and an empty stored block ends the bytes -- the form
    that can be the middle stretch of a longer stream.  needs_history: what is wrong is that nothing lies in front."""

    def __init__(self, name, fn, needs_history=False, has_open=True):
        self.name, self.needs_history = name, needs_history
        w = BitWriter()
        fn(w, True)
        self.stream = w.getvalue()
        self.open_stream = None
        if has_open and not needs_history:
            w = BitWriter()
            fn(w, False)
            stored_block(w, b"")
            self.open_stream = w.getvalue()

    def __repr__(self):
        return self.name


def _sound():
    lit = [0] * 260
    lit[256] = 3
    lit[257] = 3
    return complete(lit, range(97, 123)), [1, 1]


def reject_cases():
    if "reject" in _memo:
        return _memo["reject"]
    lit, dst = _sound()
    text = [s for s in range(256) if lit[s]] * 3
    R = []

    def add(name, fn, **kw):
        R.append(Reject(name, fn, **kw))

    def btype3(w, final):
        fixed_block(w, text, False)
        w.bits(1 if final else 0, 1)
        w.bits(3, 2)
        w.bits(0, 29)
    add("btype_3", btype3)
    add("stored_nlen_mismatch", lambda w, f: (fixed_block(w, text, False), stored_block(w, b"0123456789", f, nlen=(10 ^ 0xffff) ^ 0x100)))
    for field in (30, 31):
        add("hlit_field_%d" % field, lambda w, f, v=field: dynamic_block(w, lit, dst, text, f, hlit_field=v))
        add("hdist_field_%d" % field, lambda w, f, v=field: dynamic_block(w, lit, dst, text, f, hdist_field=v))
    used = sorted(set(lit + dst))

    def cl_with(lens_of):
        cl = [0] * 19
        for s, l in lens_of.items():
            cl[s] = l
        return cl
    over = {s: 2 for s in used}
    over[17] = 1
    add("code_length_code_oversubscribed", lambda w, f: dynamic_block(w, lit, dst, text, f, rle="none", cl_lens=cl_with(over)))
    thin = {s: 4 for s in used}
    add("code_length_code_incomplete", lambda w, f: dynamic_block(w, lit, dst, text, f, rle="none", cl_lens=cl_with(thin)))
    both = lit + dst
    add("repeat_as_first_length", lambda w, f: dynamic_block(w, lit, dst, text, f, rle=[(16, 0)] + [(l, 0) for l in both[3:]],
                                                            cl_lens=dc.flat_complete({**{s: 1 for s in used}, 16: 1})))
    n = len(both)
    add("run_overshoots_by_1", lambda w, f: dynamic_block(w, lit, dst + [0] * 9, text, f,
                                                         rle=[(l, 0) for l in both[:n - 1]] + [(1, 0), (17, 7)]))
    no_eob = list(lit)
    no_eob[255], no_eob[256] = no_eob[256], 0
    add("no_end_of_block_code", lambda w, f: dynamic_block(w, no_eob, dst, text, f, eob=False))
    fat = list(lit)
    fat[33] = 1
    add("literal_code_oversubscribed", lambda w, f: dynamic_block(w, fat, dst, text, f))
    two = [0] * 257
    two[97] = two[256] = 2
    add("literal_code_incomplete_two_codes", lambda w, f: dynamic_block(w, two, [0], [97] * 20, f))
    add("distance_code_incomplete_two_of_2_bits", lambda w, f: dynamic_block(w, lit, [2, 2], text + [(3, 1)], f))
    add("unused_half_of_a_single_distance_code",
        lambda w, f: dynamic_block(w, lit, [1], text + [(3, 1), ("L", 257, 0, 0), ("bits", 1, 1)] + text, f))
    add("length_without_any_distance_code", lambda w, f: dynamic_block(w, lit, [0], text + [("L", 257, 0, 0)] + text, f))
    for s in (286, 287):
        add("fixed_literal_length_symbol_%d" % s, lambda w, f, s=s: fixed_block(w, text + [("L", s, 0, 0)] + text, f))
    for s in (30, 31):
        add("fixed_distance_symbol_%d" % s, lambda w, f, s=s: fixed_block(w, text + [("L", 257, 0, 0), ("D", s, 0, 0)] + text, f))
    add("distance_one_beyond_the_start", lambda w, f: fixed_block(w, text + [(3, len(text) + 1)] + text, f), needs_history=True)

    def cut_in_extra_bits(w, final):
        # ... 7 bits length code 257, 5 bits distance code 29, 13 extra bits (all 0: distance 24577), end-of-block: the
        # stream stops inside the extra bits, and zeros behind it would read as a valid distance and an end-of-block code
        rng = np.random.default_rng(90)
        history(w, rng, 24600)
        fixed_block(w, text + [200] * 5 + [(3, 24577)], final)  # (five 9-bit literals: the block ends on a byte)
        assert w.bitpos % 8 == 0
        del w.out[-2:]                                      # EOB (7 bits) + 9 of the 13 extra bits
    add("input_ends_inside_extra_bits", cut_in_extra_bits, has_open=False)
    _memo["reject"] = R
    return R
