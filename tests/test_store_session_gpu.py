"""GPU: what the session layer of csrc/hpn_store.hpp decides for the store-backed families alike -- hpn_fastq_uniq_*, _uniqq_*,
_usort_*, _sort_*, _pair_*, hpn_twobit_pack_*, hpn_mrle_* and hpn_kseq_* -- on three records (ten for usort, which refuses
fewer; three of its own for mrle, whose codec knows the six symbols #/7<BF only): the byte limit, NULL text, chunks cut inside a
record, the slice copy's edges, and for sessions of two mates the mate check, the unclosed mate and the limit over both.
(hpn_rfastqc_* has its session tests in test_rqc_gpu.py: its fourth call reads typed arrays.)  Expected outputs are the Python
restatements', never the library's."""
import ctypes as C

import numpy as np
import pytest

import kseq_ref
import mrle_ref
import pair_ref
import sort_ref
import twobit_ref
import uniq_ref
import uniqq_ref
import usort_ref
from highperformancengs_amd import _lib

pytestmark = pytest.mark.gpu

THREE = b"@a\nACGT\n+\nIIII\n" b"@b\nGGCA\n+\nIIII\n" b"@c\nACGT\n+\nHHHH\n"
TEN = b"".join(b"@%c\n%s\n+\nIIII\n" % (97 + i, s) for i, s in enumerate([b"ACGT", b"GGCA", b"ACGT", b"TTTT", b"GGCA", b"ACGT", b"CCCC", b"TTTA", b"ACGT", b"GGCA"]))
MRLE3 = b"@a\nACGT\n+\n##//\n" b"@b\nGGCA\n+\n77<<\n" b"@c\nACGT\n+\nBFFF\n"      # (THREE's I and H are outside the codec's domain)
FIRST_RECORD = 15      # bytes of THREE's and TEN's first record: the cut below falls inside the second


class Family:
    """One row of the table: the raw entry points of a family under one signature, and its expected first output."""

    def __init__(self, name, prefix, result, info, mates, text, want, begin, add_mate=False, write_head=()):
        self.name, self.prefix, self.result, self.info, self.mates, self.text, self.want = name, prefix, result, info, mates, text, want
        self._begin, self.add_mate, self.write_head = begin, add_mate, write_head

    def fn(self, ctx, what):
        return getattr(ctx.L, self.prefix + "_" + what)

    def begin(self, ctx, max_bytes=0, mates=None):
        assert self.fn(ctx, "begin")(ctx.h, *self._begin(self.mates if mates is None else mates, max_bytes)) == 0

    def add(self, ctx, mate, text, last, nbytes=None):
        """(rc, info); text None: a NULL pointer with nbytes."""
        info = self.info()
        raw = np.frombuffer(text, np.uint8) if text else None
        p = C.c_void_p(raw.ctypes.data) if raw is not None and raw.size else None
        n = len(text) if nbytes is None else nbytes
        head = (mate,) if self.add_mate else ()
        return self.fn(ctx, "add")(ctx.h, *head, p, n, int(last), C.byref(info)), info

    def finish(self, ctx):
        res = self.result()
        return self.fn(ctx, "finish")(ctx.h, C.byref(res)), res

    def write(self, ctx, offset, buf, cap):
        got = C.c_uint64(7)
        p = C.c_void_p(buf.ctypes.data) if buf is not None else None
        return self.fn(ctx, "write")(ctx.h, *self.write_head, offset, p, cap, C.byref(got)), got.value

    def output(self, ctx):
        buf, parts, at = np.zeros(7, np.uint8), [], 0      # (slices of 7 bytes: the copy's offset arithmetic)
        while True:
            rc, got = self.write(ctx, at, buf, buf.size)
            assert rc == 0
            if not got:
                return b"".join(parts)
            parts.append(buf[:got].tobytes())
            at += got

    def feed_all(self, ctx, first_mate=0):
        """Every mate from first_mate on in one last chunk; the last call's info (None: no mate was left to feed)."""
        info = None
        for mate in range(first_mate, self.mates):
            rc, info = self.add(ctx, mate, self.text, True)
            assert rc == 0 and info.irregular == 0
        return info


def _uniq_want(text, paired):
    out = uniq_ref.simulate(text, text if paired else None)[0]
    return out["_1_uniq.fq" if paired else "_uniq.fq"]


def _grouping(mates, max_bytes):
    return (mates - 1, max_bytes, 0)


FAMILIES = [
    Family("uniq", "hpn_fastq_uniq", _lib.UniqResult, _lib.UniqInfo, 1, THREE, _uniq_want(THREE, False), _grouping, True, (_lib.UNIQ_TABLE_ORDER, 0)),
    Family("uniq-paired", "hpn_fastq_uniq", _lib.UniqResult, _lib.UniqInfo, 2, THREE, _uniq_want(THREE, True), _grouping, True, (_lib.UNIQ_TABLE_ORDER, 0)),
    Family("uniqq", "hpn_fastq_uniqq", _lib.UniqqResult, _lib.UniqInfo, 1, THREE, uniqq_ref.render(uniqq_ref.collapse(THREE), uniqq_ref.collapse(THREE).key_order),
           lambda mates, max_bytes: (max_bytes, 0), False, (_lib.UNIQQ_KEY_ORDER,)),
    Family("usort", "hpn_fastq_usort", _lib.UsortResult, _lib.UniqInfo, 1, TEN, usort_ref.render(usort_ref.collapse(TEN), 0), _grouping, True, (0,)),
    Family("usort-paired", "hpn_fastq_usort", _lib.UsortResult, _lib.UniqInfo, 2, TEN, usort_ref.render(usort_ref.collapse(TEN, TEN), 0), _grouping, True, (0,)),
    Family("sort", "hpn_fastq_sort", _lib.SortResult, _lib.SortInfo, 1, THREE, sort_ref.simulate(THREE, False, r=1 << 40)[0],
           lambda mates, max_bytes: (0, max_bytes)),
    Family("twobit", "hpn_twobit_pack", _lib.TwobitResult, _lib.SortInfo, 1, THREE, twobit_ref.pack(THREE)[0], lambda mates, max_bytes: (max_bytes,)),
    Family("pair", "hpn_fastq_pair", _lib.PairResult, _lib.SortInfo, 2, THREE, pair_ref.outputs(THREE, THREE, pair_ref.device(THREE, THREE)[1])[0],
           lambda mates, max_bytes: (max_bytes,), True, (0,)),
    Family("mrle", "hpn_mrle", _lib.MrleResult, _lib.SortInfo, 1, MRLE3, mrle_ref.mrle(MRLE3)[0][mrle_ref.PACKED], lambda mates, max_bytes: (max_bytes,),
           False, (_lib.MRLE_PACKED,)),
    Family("kseq", "hpn_kseq", _lib.KseqResult, _lib.SortInfo, 1, THREE, kseq_ref.map_kseq(THREE)[0], lambda mates, max_bytes: (max_bytes,)),
]
PAIRED = [f for f in FAMILIES if f.mates == 2]
by_name = dict(argvalues=FAMILIES, ids=[f.name for f in FAMILIES])


@pytest.fixture(scope="module")
def ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


def test_the_inputs_are_the_issue_s():
    assert THREE.count(b"\n") == 12 and max(len(r) for r in THREE.split(b"@")[1:]) + 1 <= 20 and TEN.count(b"\n") == 40
    assert all(t[FIRST_RECORD - 1:FIRST_RECORD + 1] == b"\n@" for t in (THREE, TEN)) and all(f.want for f in FAMILIES)


@pytest.mark.parametrize("fam", **by_name)
def test_limit_closes_and_begin_reopens(ctx, fam):
    n = len(fam.text)
    fam.begin(ctx, max_bytes=n - 1)
    rc, _ = fam.add(ctx, 0, fam.text, True)
    assert rc == _lib.E_CAPACITY and str(n).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
    assert fam.finish(ctx)[0] == _lib.E_STATE
    fam.begin(ctx, max_bytes=n * fam.mates)
    fam.feed_all(ctx)
    assert fam.finish(ctx)[0] == 0 and fam.output(ctx) == fam.want


@pytest.mark.parametrize("fam", **by_name)
def test_null_text_leaves_the_session_open(ctx, fam):
    fam.begin(ctx)
    assert fam.add(ctx, 0, None, True, nbytes=len(fam.text))[0] == _lib.E_ARG
    info = fam.feed_all(ctx)
    assert info.n_records == fam.text.count(b"\n") // 4
    assert fam.finish(ctx)[0] == 0 and fam.output(ctx) == fam.want


@pytest.mark.parametrize("fam", **by_name)
def test_chunks_cut_inside_a_record(ctx, fam):
    cut, whole = FIRST_RECORD + 5, fam.text.count(b"\n") // 4
    fam.begin(ctx)
    fam.feed_all(ctx)
    assert fam.finish(ctx)[0] == 0
    one_chunk = fam.output(ctx)
    fam.begin(ctx)
    n = 0
    for piece, last in ((fam.text[:cut], False), (fam.text[cut:], False), (b"", True)):
        rc, info = fam.add(ctx, 0, piece, last)
        assert rc == 0 and info.irregular == 0
        n += info.n_records
    assert n == whole
    fam.feed_all(ctx, first_mate=1)
    assert fam.finish(ctx)[0] == 0 and fam.output(ctx) == one_chunk == fam.want


@pytest.mark.parametrize("fam", **by_name)
def test_write_edges(ctx, fam):
    fam.begin(ctx)
    fam.feed_all(ctx)
    assert fam.finish(ctx)[0] == 0
    total, buf = len(fam.want), np.zeros(16, np.uint8)
    assert fam.write(ctx, total, buf, 16) == (0, 0)
    assert fam.write(ctx, total + 1, buf, 16)[0] == _lib.E_ARG
    assert fam.write(ctx, 0, buf, 0) == (0, 0)
    assert fam.write(ctx, 0, None, 16)[0] == _lib.E_ARG
    k = min(total, 16)
    assert fam.write(ctx, 0, buf, 16) == (0, k) and buf[:k].tobytes() == fam.want[:k]


@pytest.mark.parametrize("fam", PAIRED, ids=[f.name for f in PAIRED])
def test_two_mates(ctx, fam):
    n = len(fam.text)
    if fam.name == "pair":      # (every session has both mates: the mate behind them)
        fam.begin(ctx)
        assert fam.add(ctx, 2, fam.text, True)[0] == _lib.E_ARG
    else:
        fam.begin(ctx, mates=1)
        assert fam.add(ctx, 1, fam.text, True)[0] == _lib.E_ARG
    fam.begin(ctx)
    assert fam.add(ctx, 0, fam.text, True)[0] == 0
    assert fam.finish(ctx)[0] == _lib.E_STATE      # mate 1 has not had its last chunk
    fam.begin(ctx, max_bytes=2 * n - 1)
    assert fam.add(ctx, 0, fam.text, True)[0] == 0
    assert fam.add(ctx, 1, fam.text, True)[0] == _lib.E_CAPACITY and str(2 * n).encode() in ctx.L.hpn_ctx_last_error(ctx.h)
    assert fam.finish(ctx)[0] == _lib.E_STATE
