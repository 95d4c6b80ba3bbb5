"""Thin Python view of the C ABI, used by tests and bench.py.

The drop-in surface of this project is the C ABI (include/hpngs.h) and the CLI
tools built on it (csrc/tools); this module only moves pointers.  Host arrays are
numpy, device arrays are anything with ``data_ptr()`` (torch tensors) or an int
address.  Every failure raises ``HpnError``; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import HpnError, Tally


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    raise TypeError(type(x))


class TallyResult:
    """Accumulators of count_read (fastq_count_kthread.c:116): numpy views over an hpn_tally."""

    def __init__(self, qual_hist=False, nuc_hist=False):
        self.c = Tally()
        self.qual_hist = np.zeros((_lib.QUAL_ROWS, _lib.LEN_BINS), np.uint64) if qual_hist else None
        self.nuc_hist = np.zeros((_lib.NUC_CODES, _lib.LEN_BINS), np.uint64) if nuc_hist else None
        if qual_hist:
            self.c.qual_hist = self.qual_hist.ctypes.data_as(C.POINTER(C.c_uint64))
        if nuc_hist:
            self.c.nuc_hist = self.nuc_hist.ctypes.data_as(C.POINTER(C.c_uint64))

    @property
    def seqlen(self):
        return np.frombuffer(self.c.seqlen, dtype=np.uint64)

    @property
    def total(self):
        return int(self.c.total)

    @property
    def q20(self):
        return int(self.c.q20)

    @property
    def q30(self):
        return int(self.c.q30)


class Context:
    """One per GPU (hpn_ctx)."""

    def __init__(self, device=0):
        self.L = _lib.lib()
        h = C.c_void_p()
        rc = self.L.hpn_ctx_create(device, C.byref(h))
        if rc != 0:
            raise HpnError(rc, "hpn_ctx_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.hpn_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise HpnError(rc, what, self.L.hpn_ctx_last_error(self.h).decode())

    def set_stream(self, hip_stream):
        self._ck(self.L.hpn_ctx_set_stream(self.h, C.c_void_p(hip_stream) if hip_stream else None), "set_stream")

    def sync(self):
        self._ck(self.L.hpn_ctx_sync(self.h), "sync")

    def last_kernel_ms(self, family=0):
        ms = C.c_float()
        self._ck(self.L.hpn_ctx_last_kernel_ms(self.h, family, C.byref(ms)), "last_kernel_ms")
        return ms.value

    # ---- fastq_count ------------------------------------------------------
    def fastq_tally(self, qual, off, base=None, acc=None, qual_hist=False, nuc_hist=False):
        """Host batch -> adds into `acc` (new TallyResult if None). Mirrors count_read."""
        qual = np.ascontiguousarray(qual, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        if base is not None:
            base = np.ascontiguousarray(base, np.uint8)
        if acc is None:
            acc = TallyResult(qual_hist, nuc_hist)
        self._ck(self.L.hpn_fastq_tally(self.h, _ptr(qual), _ptr(base), _ptr(off), len(off) - 1, C.byref(acc.c)),
                 "hpn_fastq_tally")
        return acc

    def fastq_tally_dev(self, d_qual, d_off, n, d_base=None, flags=0):
        self._ck(self.L.hpn_fastq_tally_dev(self.h, _ptr(d_qual), _ptr(d_base), _ptr(d_off), n, flags),
                 "hpn_fastq_tally_dev")

    def fastq_tally_fetch(self, acc=None, qual_hist=False, nuc_hist=False):
        if acc is None:
            acc = TallyResult(qual_hist, nuc_hist)
        self._ck(self.L.hpn_fastq_tally_fetch(self.h, C.byref(acc.c)), "hpn_fastq_tally_fetch")
        return acc

    def tally_devptr(self):
        p = C.c_void_p()
        self._ck(self.L.hpn_fastq_tally_devptr(self.h, C.byref(p)), "hpn_fastq_tally_devptr")
        return p.value

    # ---- R plugin tally (Rgzfastq_uniq.c) -----------------------------------
    def fastq_rqc(self, seq, qual, off, out=None):
        """-> dict(quality int32[300,128] view of [q+128*pos], nucleotide int32[300,5], length int32[300], gc f64[n]);
        pass the previous dict as `out` to keep adding into the matrices."""
        seq = np.ascontiguousarray(seq, np.uint8)
        qual = np.ascontiguousarray(qual, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        M = _lib.RQC_MAXLEN
        out = out or {"quality": np.zeros((M, 128), np.int32), "nucleotide": np.zeros((M, 5), np.int32),
                      "length": np.zeros(M, np.int32)}
        out["gc"] = np.zeros(max(n, 1), np.float64)
        r = _lib.Rqc()
        i32 = C.POINTER(C.c_int32)
        r.quality, r.nucleotide = out["quality"].ctypes.data_as(i32), out["nucleotide"].ctypes.data_as(i32)
        r.length, r.gc = out["length"].ctypes.data_as(i32), out["gc"].ctypes.data_as(C.POINTER(C.c_double))
        self._ck(self.L.hpn_fastq_rqc(self.h, _ptr(seq), _ptr(qual), _ptr(off), n, C.byref(r)), "hpn_fastq_rqc")
        out["gc"] = out["gc"][:n]
        return out

    def fastq_read_gc_dev(self, d_seq, d_off, n, d_gc):
        self._ck(self.L.hpn_fastq_read_gc_dev(self.h, _ptr(d_seq), _ptr(d_off), n, _ptr(d_gc)), "hpn_fastq_read_gc_dev")

    # ---- fastq_trim -------------------------------------------------------
    def fastq_trim(self, seq, qual, off, S, E):
        seq = np.ascontiguousarray(seq, np.uint8)
        qual = np.ascontiguousarray(qual, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        cap = max(int(off[-1] - off[0]), 1)
        oseq, oqual, ooff = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64)
        self._ck(self.L.hpn_fastq_trim(self.h, _ptr(seq), _ptr(qual), _ptr(off), n, S, E, _ptr(oseq), _ptr(oqual),
                                       _ptr(ooff)), "hpn_fastq_trim")
        tot = int(ooff[-1])
        return oseq[:tot], oqual[:tot], ooff

    def fastq_trim_dev(self, d_seq, d_qual, d_off, n, S, E, d_out_seq, d_out_qual, d_out_off):
        self._ck(self.L.hpn_fastq_trim_dev(self.h, _ptr(d_seq), _ptr(d_qual), _ptr(d_off), n, S, E, _ptr(d_out_seq),
                                           _ptr(d_out_qual), _ptr(d_out_off)), "hpn_fastq_trim_dev")

    def fastq_trim_points_dev(self, d_seq, d_qual, d_off, n, d_beg, d_end, d_out_seq, d_out_qual, d_out_off):
        self._ck(self.L.hpn_fastq_trim_points_dev(self.h, _ptr(d_seq), _ptr(d_qual), _ptr(d_off), n, _ptr(d_beg), _ptr(d_end),
                                                  _ptr(d_out_seq), _ptr(d_out_qual), _ptr(d_out_off)), "hpn_fastq_trim_points_dev")

    def fastq_qtrim_points_dev(self, d_qual, d_off, n, threshold, d_beg, d_end):
        self._ck(self.L.hpn_fastq_qtrim_points_dev(self.h, _ptr(d_qual), _ptr(d_off), n, threshold, _ptr(d_beg), _ptr(d_end)),
                 "hpn_fastq_qtrim_points_dev")

    # ---- extension: quality-threshold trim points --------------------------
    def fastq_qtrim_points(self, qual, off, threshold):
        qual = np.ascontiguousarray(qual, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        beg, end = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        self._ck(self.L.hpn_fastq_qtrim_points(self.h, _ptr(qual), _ptr(off), n, threshold, _ptr(beg), _ptr(end)),
                 "hpn_fastq_qtrim_points")
        return beg[:n], end[:n]

    def fastq_trim_points(self, seq, qual, off, beg, end):
        seq = np.ascontiguousarray(seq, np.uint8)
        qual = np.ascontiguousarray(qual, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        beg, end = np.ascontiguousarray(beg, np.uint32), np.ascontiguousarray(end, np.uint32)
        n = len(off) - 1
        cap = max(int(off[-1] - off[0]), 1)
        oseq, oqual, ooff = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64)
        self._ck(self.L.hpn_fastq_trim_points(self.h, _ptr(seq), _ptr(qual), _ptr(off), n, _ptr(beg), _ptr(end),
                                              _ptr(oseq), _ptr(oqual), _ptr(ooff)), "hpn_fastq_trim_points")
        tot = int(ooff[-1])
        return oseq[:tot], oqual[:tot], ooff

    # ---- raw-text front end (device-side framing) ------------------------------
    def text_begin(self):
        self._ck(self.L.hpn_fastq_text_begin(self.h), "hpn_fastq_text_begin")

    @staticmethod
    def _text(chunk):
        if isinstance(chunk, (bytes, bytearray, memoryview)):
            chunk = np.frombuffer(chunk, np.uint8)
        if isinstance(chunk, np.ndarray):
            chunk = np.ascontiguousarray(chunk, np.uint8)
            return chunk, chunk.size
        return chunk, chunk.numel()  # device tensor

    def text_count(self, chunk, last=False, flags=0):
        """One chunk of FASTQ text -> device accumulators; returns the hpn_text_info."""
        chunk, n = self._text(chunk)
        info = _lib.TextInfo()
        self._ck(self.L.hpn_fastq_text_count(self.h, _ptr(chunk) if n else None, n, int(bool(last)), flags, C.byref(info)),
                 "hpn_fastq_text_count")
        return info

    def text_count_inplace(self, d_text, nbytes, last=False, flags=0):
        """A chunk of FASTQ text that lies on the device, framed where it lies (8192 writable bytes in front of d_text)."""
        info = _lib.TextInfo()
        self._ck(self.L.hpn_fastq_text_count_inplace(self.h, _ptr(d_text) if d_text is not None else None, int(nbytes), int(bool(last)), flags,
                                                     C.byref(info)), "hpn_fastq_text_count_inplace")
        return info

    def text_records(self, chunk, last=False):
        """One chunk of FASTQ text -> hpn_text_info with the records it completes (gzfastq_sample's count_read)."""
        chunk, n = self._text(chunk)
        info = _lib.TextInfo()
        self._ck(self.L.hpn_fastq_text_records(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)),
                 "hpn_fastq_text_records")
        return info

    def text_trim(self, chunk, S, E, last=False):
        """One chunk of FASTQ text -> (trimmed text bytes, hpn_text_info)."""
        chunk, n = self._text(chunk)
        info = _lib.TextInfo()
        out = np.zeros(n + 8192, np.uint8)
        self._ck(self.L.hpn_fastq_text_trim(self.h, _ptr(chunk) if n else None, n, int(bool(last)), S, E, _ptr(out), out.size,
                                            C.byref(info)), "hpn_fastq_text_trim")
        return out[:0 if info.irregular else int(info.n_bytes)].tobytes(), info

    def fastq_text_sample(self, chunk, last=False, *, threshold=None, seed_add=0, picks=None, fasta=False, first_ordinal=0, out_cap=None):
        """One chunk of FASTQ text -> (sampled text bytes, kept 0-based ordinals, hpn_sample_info): hpn_fastq_text_sample.
        Exactly one rule: `threshold` (0 .. 2^24, with `seed_add`) or `picks` (sorted uint64 ordinals over the whole stream)."""
        if (threshold is None) == (picks is None):
            raise ValueError("give threshold= or picks=")
        chunk, n = self._text(chunk)
        rule = _lib.SampleRule(fasta=int(bool(fasta)), first_ordinal=first_ordinal)
        if picks is None:
            rule.mode, rule.seed_add, rule.threshold = _lib.SAMPLE_FRACTION, seed_add & 0xFFFFFFFF, threshold
        else:
            picks = np.ascontiguousarray(picks, np.uint64)
            rule.mode, rule.picks, rule.n_picks = _lib.SAMPLE_PICKS, picks.ctypes.data if picks.size else None, picks.size
        info = _lib.SampleInfo()
        out = np.zeros(7 * (n + 8192) if out_cap is None else out_cap, np.uint8)
        kept = np.zeros((n + 8192) // 4, np.uint64)
        self._ck(self.L.hpn_fastq_text_sample(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(rule), _ptr(out) if out.size else None,
                                              out.size, _ptr(kept), kept.size, C.byref(info)), "hpn_fastq_text_sample")
        if info.irregular:
            return b"", kept[:0], info
        return out[:int(info.n_bytes)].tobytes(), kept[:int(info.n_kept)].copy(), info

    # ---- duplicate removal (gzfastq_uniq) ------------------------------------------------
    def uniq_begin(self, paired=False, max_bytes=0, hash_bits=0):
        self._ck(self.L.hpn_fastq_uniq_begin(self.h, int(bool(paired)), int(max_bytes), int(hash_bits)), "hpn_fastq_uniq_begin")

    def uniq_add(self, chunk, mate=0, last=False):
        """One chunk of FASTQ text of one mate into the session's device store; returns the hpn_uniq_info."""
        chunk, n = self._text(chunk)
        info = _lib.UniqInfo()
        self._ck(self.L.hpn_fastq_uniq_add(self.h, int(mate), _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_fastq_uniq_add")
        return info

    def uniq_finish(self):
        res = _lib.UniqResult()
        self._ck(self.L.hpn_fastq_uniq_finish(self.h, C.byref(res)), "hpn_fastq_uniq_finish")
        return res

    def uniq_output(self, which=_lib.UNIQ_TABLE_ORDER, mate=0, slice_bytes=1 << 24):
        """The whole text of one output, fetched in slices (hpn_fastq_uniq_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_fastq_uniq_write(self.h, int(which), int(mate), at, _ptr(buf), buf.size, C.byref(got)), "hpn_fastq_uniq_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    # ---- duplicate removal, most frequent first (gzfastq_uniq_sort) ---------------------------
    def usort_begin(self, paired=False, max_bytes=0, hash_bits=0):
        self._ck(self.L.hpn_fastq_usort_begin(self.h, int(bool(paired)), int(max_bytes), int(hash_bits)), "hpn_fastq_usort_begin")

    def usort_add(self, chunk, mate=0, last=False):
        """One chunk of FASTQ text of one mate into the session's device store; returns the hpn_uniq_info."""
        chunk, n = self._text(chunk)
        info = _lib.UniqInfo()
        self._ck(self.L.hpn_fastq_usort_add(self.h, int(mate), _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_fastq_usort_add")
        return info

    def usort_finish(self):
        """The hpn_usort_result.  Where the reference has no answer (HPN_E_DOMAIN) the result comes back with no_answer set
        instead of an exception: there is no output then."""
        res = _lib.UsortResult()
        rc = self.L.hpn_fastq_usort_finish(self.h, C.byref(res))
        if not (rc == _lib.E_DOMAIN and res.no_answer):
            self._ck(rc, "hpn_fastq_usort_finish")
        return res

    def usort_output(self, mate=0, slice_bytes=1 << 24):
        """The whole text of one mate's output, fetched in slices (hpn_fastq_usort_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_fastq_usort_write(self.h, int(mate), at, _ptr(buf), buf.size, C.byref(got)), "hpn_fastq_usort_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    # ---- duplicate removal that keeps every quality line (gzfastq_uniqQ) ----------------------
    def uniqq_begin(self, max_bytes=0, hash_bits=0):
        self._ck(self.L.hpn_fastq_uniqq_begin(self.h, int(max_bytes), int(hash_bits)), "hpn_fastq_uniqq_begin")

    def uniqq_add(self, chunk, last=False):
        """One chunk of FASTQ text into the session's device store; returns the hpn_uniq_info."""
        chunk, n = self._text(chunk)
        info = _lib.UniqInfo()
        self._ck(self.L.hpn_fastq_uniqq_add(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_fastq_uniqq_add")
        return info

    def uniqq_finish(self):
        res = _lib.UniqqResult()
        self._ck(self.L.hpn_fastq_uniqq_finish(self.h, C.byref(res)), "hpn_fastq_uniqq_finish")
        return res

    def uniqq_output(self, which=_lib.UNIQQ_KEY_ORDER, slice_bytes=1 << 24):
        """The whole text of one output, fetched in slices (hpn_fastq_uniqq_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_fastq_uniqq_write(self.h, int(which), at, _ptr(buf), buf.size, C.byref(got)), "hpn_fastq_uniqq_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    # ---- the whole file ordered by name or sequence (gzfastq_sort) ---------------------------
    def sort_begin(self, by_name=False, max_bytes=0):
        self._ck(self.L.hpn_fastq_sort_begin(self.h, int(bool(by_name)), int(max_bytes)), "hpn_fastq_sort_begin")

    def sort_add(self, chunk, last=False):
        """One chunk of FASTQ text into the session's device store; returns the hpn_sort_info."""
        chunk, n = self._text(chunk)
        info = _lib.SortInfo()
        self._ck(self.L.hpn_fastq_sort_add(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_fastq_sort_add")
        return info

    def sort_finish(self):
        res = _lib.SortResult()
        self._ck(self.L.hpn_fastq_sort_finish(self.h, C.byref(res)), "hpn_fastq_sort_finish")
        return res

    def sort_output(self, slice_bytes=1 << 24):
        """The whole sorted text, fetched in slices (hpn_fastq_sort_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_fastq_sort_write(self.h, at, _ptr(buf), buf.size, C.byref(got)), "hpn_fastq_sort_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    # ---- kseq input, the first record of every distinct sequence in the sequences' order (map_kseq, kbtree_kseq) ----
    def kseq_begin(self, max_bytes=0):
        self._ck(self.L.hpn_kseq_begin(self.h, int(max_bytes)), "hpn_kseq_begin")

    def kseq_add(self, chunk, last=False):
        """One chunk of FASTA or FASTQ text, cut anywhere, into the session's device store; returns the hpn_sort_info.
        info.irregular (TEXT_KSEQ: neither of the two shapes the device frames; TEXT_NUL) closes the session."""
        chunk, n = self._text(chunk)
        info = _lib.SortInfo()
        self._ck(self.L.hpn_kseq_add(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_kseq_add")
        return info

    def kseq_finish(self):
        res = _lib.KseqResult()
        self._ck(self.L.hpn_kseq_finish(self.h, C.byref(res)), "hpn_kseq_finish")
        return res

    def kseq_output(self, slice_bytes=1 << 24):
        """The whole output text, fetched in slices (hpn_kseq_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_kseq_write(self.h, at, _ptr(buf), buf.size, C.byref(got)), "hpn_kseq_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    # ---- the sequences packed to 2 bits per base, and back (fastq2twobit, twoBit2seq) ---------
    def twobit_pack_begin(self, max_bytes=0):
        self._ck(self.L.hpn_twobit_pack_begin(self.h, int(max_bytes)), "hpn_twobit_pack_begin")

    def twobit_pack_add(self, chunk, last=False):
        """One chunk of FASTQ text into the session's device store; returns the hpn_sort_info."""
        chunk, n = self._text(chunk)
        info = _lib.SortInfo()
        self._ck(self.L.hpn_twobit_pack_add(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_twobit_pack_add")
        return info

    def twobit_pack_finish(self):
        res = _lib.TwobitResult()
        self._ck(self.L.hpn_twobit_pack_finish(self.h, C.byref(res)), "hpn_twobit_pack_finish")
        return res

    def twobit_pack_output(self, slice_bytes=1 << 24):
        """The whole packed output, fetched in slices (hpn_twobit_pack_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_twobit_pack_write(self.h, at, _ptr(buf), buf.size, C.byref(got)), "hpn_twobit_pack_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    def twobit_unpack(self, seq_len, packed_len, packed, n_records, out=None):
        """n_records records of packed_len bytes -> text (hpn_twobit_unpack).  packed: bytes / numpy (host) or a device array; out: None
        (a host buffer is made and its bytes returned) or a device array of enough bytes (returns the byte count)."""
        if isinstance(packed, (bytes, bytearray)):
            packed = np.frombuffer(bytes(packed), np.uint8)
        need = int(n_records) * (int(seq_len) + 1)
        got = C.c_uint64(0)
        if out is None:
            buf = np.zeros(max(need, 1), np.uint8)
            self._ck(self.L.hpn_twobit_unpack(self.h, int(seq_len), int(packed_len), _ptr(packed), int(n_records), _ptr(buf), need, C.byref(got)), "hpn_twobit_unpack")
            return buf[:got.value].tobytes()
        self._ck(self.L.hpn_twobit_unpack(self.h, int(seq_len), int(packed_len), _ptr(packed), int(n_records), _ptr(out), int(out.numel() * out.element_size()),
                                          C.byref(got)), "hpn_twobit_unpack")
        return got.value

    # ---- the quality lines run-length packed, and decoded again (gzfastq_mrle) ------------------
    def mrle_begin(self, max_bytes=0):
        self._ck(self.L.hpn_mrle_begin(self.h, int(max_bytes)), "hpn_mrle_begin")

    def mrle_add(self, chunk, last=False):
        """One chunk of FASTQ text into the session's device store; returns the hpn_sort_info."""
        chunk, n = self._text(chunk)
        info = _lib.SortInfo()
        self._ck(self.L.hpn_mrle_add(self.h, _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_mrle_add")
        return info

    def mrle_finish(self):
        res = _lib.MrleResult()
        self._ck(self.L.hpn_mrle_finish(self.h, C.byref(res)), "hpn_mrle_finish")
        return res

    def mrle_output(self, which, slice_bytes=1 << 24):
        """One whole output (_lib.MRLE_PACKED / _TEXT / _SHARED), fetched in slices (hpn_mrle_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_mrle_write(self.h, int(which), at, _ptr(buf), buf.size, C.byref(got)), "hpn_mrle_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    # ---- Rfastqc.R's qsort_hash_count from FASTQ text (rfastqc_tally) ----------------------------
    def rfastqc_begin(self, paired=False, max_bytes=0, hash_bits=0):
        self._ck(self.L.hpn_rfastqc_begin(self.h, int(bool(paired)), int(max_bytes), int(hash_bits)), "hpn_rfastqc_begin")

    def rfastqc_add(self, mate, chunk, last=False):
        """One chunk of mate 0 or 1 into that mate's device store; returns the hpn_sort_info."""
        chunk, n = self._text(chunk)
        info = _lib.SortInfo()
        self._ck(self.L.hpn_rfastqc_add(self.h, int(mate), _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_rfastqc_add")
        return info

    def rfastqc_finish(self):
        res = _lib.RfastqcResult()
        self._ck(self.L.hpn_rfastqc_finish(self.h, C.byref(res)), "hpn_rfastqc_finish")
        return res

    def rfastqc_array(self, which, mate=0, slice_elems=1 << 22):
        """One whole array (_lib.RFASTQC_*) of a finished session as numpy, fetched in slices (hpn_rfastqc_read)."""
        buf = np.zeros(max(int(slice_elems), 1), np.float64 if which == _lib.RFASTQC_GC else np.int32)
        parts, at = [], 0
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_rfastqc_read(self.h, int(which), int(mate), at, _ptr(buf), buf.size, C.byref(got)), "hpn_rfastqc_read")
            if not got.value:
                return np.concatenate(parts) if parts else buf[:0].copy()
            parts.append(buf[:got.value].copy())
            at += got.value

    def rfastqc(self, fq1, fq2=None, hash_bits=0):
        """qsort_hash_count(fq1, fq2) over FASTQ text held in memory: (result, list) with the list's 5 (9) elements as numpy arrays --
        the duplicate counts, then gc, quality, nucleotide, length of mate 1 (and of mate 2)."""
        self.rfastqc_begin(fq2 is not None, hash_bits=hash_bits)
        self.rfastqc_add(0, fq1, last=True)
        if fq2 is not None:
            self.rfastqc_add(1, fq2, last=True)
        res = self.rfastqc_finish()
        out = [self.rfastqc_array(_lib.RFASTQC_DUP)]
        for mate in range(2 if fq2 is not None else 1):
            out += [self.rfastqc_array(w, mate) for w in (_lib.RFASTQC_GC, _lib.RFASTQC_QUALITY, _lib.RFASTQC_NUCLEOTIDE, _lib.RFASTQC_LENGTH)]
        return res, out

    # ---- two files split into pairs and singles (pick_pair) ------------------------------------
    def fastq_pair_begin(self, max_bytes=0):
        self._ck(self.L.hpn_fastq_pair_begin(self.h, int(max_bytes)), "hpn_fastq_pair_begin")

    def fastq_pair_add(self, mate, chunk, last=False):
        """One chunk of READ1 (mate 0) or READ2 (mate 1) into that mate's device store; returns the hpn_sort_info."""
        chunk, n = self._text(chunk)
        info = _lib.SortInfo()
        self._ck(self.L.hpn_fastq_pair_add(self.h, int(mate), _ptr(chunk) if n else None, n, int(bool(last)), C.byref(info)), "hpn_fastq_pair_add")
        return info

    def fastq_pair_finish(self):
        """The hpn_pair_result.  Where neither proposal verifies (HPN_E_DOMAIN) the result comes back with unverified set instead
        of an exception: there is no output then."""
        res = _lib.PairResult()
        rc = self.L.hpn_fastq_pair_finish(self.h, C.byref(res))
        if not (rc == _lib.E_DOMAIN and res.unverified):
            self._ck(rc, "hpn_fastq_pair_finish")
        return res

    def fastq_pair_output(self, which, slice_bytes=1 << 24):
        """One of the four outputs (0 _1_PE, 1 _1_SE, 2 _2_PE, 3 _2_SE), fetched in slices (hpn_fastq_pair_write)."""
        parts, at = [], 0
        buf = np.zeros(max(int(slice_bytes), 1), np.uint8)
        while True:
            got = C.c_uint64(0)
            self._ck(self.L.hpn_fastq_pair_write(self.h, int(which), at, _ptr(buf), buf.size, C.byref(got)), "hpn_fastq_pair_write")
            if not got.value:
                return b"".join(parts)
            parts.append(buf[:got.value].tobytes())
            at += got.value

    def sort_pairs(self, keys, vals):
        """Stable ascending sort of uint64 keys with their uint32 payload on the device (hpn_sort_pairs_u64); returns copies."""
        keys, vals = np.array(keys, np.uint64), np.array(vals, np.uint32)
        assert keys.shape == vals.shape and keys.ndim == 1
        self._ck(self.L.hpn_sort_pairs_u64(self.h, _ptr(keys) if keys.size else None, _ptr(vals) if keys.size else None, keys.size), "hpn_sort_pairs_u64")
        return keys, vals

    def sort_pairs_bits(self, keys, vals, begin_bit, end_bit):
        """sort_pairs by the key bits [begin_bit, end_bit) only (hpn_sort_pairs_u64_bits); returns copies."""
        keys, vals = np.array(keys, np.uint64), np.array(vals, np.uint32)
        assert keys.shape == vals.shape and keys.ndim == 1
        self._ck(self.L.hpn_sort_pairs_u64_bits(self.h, _ptr(keys) if keys.size else None, _ptr(vals) if keys.size else None, keys.size,
                                                int(begin_bit), int(end_bit)), "hpn_sort_pairs_u64_bits")
        return keys, vals

    def sort_pairs_digits(self, keys, vals, digits):
        """sort_pairs by the key bytes whose bit is set in digits (hpn_sort_pairs_u64_digits); returns copies."""
        keys, vals = np.array(keys, np.uint64), np.array(vals, np.uint32)
        assert keys.shape == vals.shape and keys.ndim == 1
        self._ck(self.L.hpn_sort_pairs_u64_digits(self.h, _ptr(keys) if keys.size else None, _ptr(vals) if keys.size else None, keys.size,
                                                  int(digits)), "hpn_sort_pairs_u64_digits")
        return keys, vals

    def excl_scan(self, values, out_bits=None):
        """The n + 1 exclusive prefix sums of a uint32 or uint64 array on the device (hpn_excl_scan), as uint32 (modulo 2^32)
        or uint64; out_bits defaults to the input's width."""
        values = np.ascontiguousarray(values)
        assert values.ndim == 1 and values.dtype in (np.uint32, np.uint64)
        in_bits = values.dtype.itemsize * 8
        out_bits = in_bits if out_bits is None else int(out_bits)
        out = np.empty(values.size + 1, np.uint32 if out_bits == 32 else np.uint64)
        self._ck(self.L.hpn_excl_scan(self.h, _ptr(values) if values.size else None, in_bits, _ptr(out), out_bits, values.size), "hpn_excl_scan")
        return out

    # ---- one stream framed by several contexts: pieces ---------------------------------
    def text_piece_lines(self, text, head, own_bytes, last=False):
        """First half of a piece (hpn_fastq_text_piece_lines): text = head byte + piece + tail; returns hpn_text_piece."""
        text, n = self._text(text)
        out = _lib.TextPiece()
        self._ck(self.L.hpn_fastq_text_piece_lines(self.h, _ptr(text) if n else None, n, head, own_bytes, int(bool(last)), C.byref(out)),
                 "hpn_fastq_text_piece_lines")
        return out

    def text_piece_count(self, lines_before, flags=0):
        info = _lib.TextInfo()
        self._ck(self.L.hpn_fastq_text_piece_count(self.h, lines_before, flags, C.byref(info)), "hpn_fastq_text_piece_count")
        return info

    def text_piece_trim(self, lines_before, S, E, cap):
        info = _lib.TextInfo()
        out = np.zeros(cap, np.uint8)
        self._ck(self.L.hpn_fastq_text_piece_trim(self.h, lines_before, S, E, _ptr(out), out.size, C.byref(info)), "hpn_fastq_text_piece_trim")
        return out[:0 if info.irregular else int(info.n_bytes)].tobytes(), info

    # ---- BGZF inflate on the device ----------------------------------------------
    def bgzf_inflate_dev(self, d_comp, d_blocks, n_blocks, d_out, d_status):
        self._ck(self.L.hpn_bgzf_inflate_dev(self.h, _ptr(d_comp), _ptr(d_blocks), n_blocks, _ptr(d_out), _ptr(d_status)),
                 "hpn_bgzf_inflate_dev")

    # ---- one gzip member on the device (two passes) -------------------------------
    def gz_inflate_dev(self, d_comp, d_chunks, n_chunks, sym_cap, d_text, text_cap, d_window_in=None, d_window_out=None):
        """hpn_gz_inflate_dev; returns hpn_gz_info (status != 0: a stretch could not be decoded as given)."""
        info = _lib.GzInfo()
        self._ck(self.L.hpn_gz_inflate_dev(self.h, _ptr(d_comp), _ptr(d_chunks), n_chunks, sym_cap,
                                           _ptr(d_window_in) if d_window_in is not None else None, _ptr(d_text) if d_text is not None else None,
                                           text_cap, _ptr(d_window_out) if d_window_out is not None else None, C.byref(info)),
                 "hpn_gz_inflate_dev")
        return info

    def gz_members(self):
        """hpn_gz_members: [(text_end, isize)] of the members that ended inside the last hpn_gz_inflate_dev call."""
        n = C.c_uint32(0)
        rc = self.L.hpn_gz_members(self.h, None, 0, C.byref(n))
        if n.value == 0:
            self._ck(rc, "hpn_gz_members")
            return []
        buf = np.zeros(n.value, np.dtype([("text_end", "<u8"), ("isize", "<u4"), ("reserved", "<u4")]))
        self._ck(self.L.hpn_gz_members(self.h, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "hpn_gz_members")
        return [(int(r["text_end"]), int(r["isize"])) for r in buf]

    def crc32_dev(self, d_data, spans):
        """CRC-32 of d_data[off : off + len) for every (off, len) in spans (hpn_crc32_dev) -> list of ints."""
        n = len(spans)
        arr = np.array(spans, np.uint64).reshape(-1, 2) if n else np.zeros((0, 2), np.uint64)
        out = np.zeros(max(n, 1), np.uint32)
        self._ck(self.L.hpn_crc32_dev(self.h, _ptr(d_data), _ptr(arr) if n else None, n, _ptr(out)), "hpn_crc32_dev")
        return [int(x) for x in out[:n]]

    def gz_find_starts_dev(self, d_comp, comp_bytes, slices):
        """First block start (bit position in d_comp) in every (lo_bit, n_bits) slice, or 2^64 - 1 (hpn_gz_find_starts_dev)."""
        n = len(slices)
        arr = np.array(slices, np.uint64).reshape(-1, 2) if n else np.zeros((0, 2), np.uint64)
        out = np.zeros(max(n, 1), np.uint64)
        self._ck(self.L.hpn_gz_find_starts_dev(self.h, _ptr(d_comp), int(comp_bytes), _ptr(arr) if n else None, n, _ptr(out)), "hpn_gz_find_starts_dev")
        return out[:n]

    # ---- BAM --------------------------------------------------------------
    @staticmethod
    def _batch(soa, keep):
        """hpn_bam_batch over numpy arrays / device tensors; `keep` pins the temporaries."""
        b = _lib.BamBatch()
        b.n = len(soa.tid)
        for f in ("tid", "pos", "flag", "l_qseq", "cigar_off", "cigar", "seq_off", "seq4"):
            a = getattr(soa, f, None)
            if a is not None and isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                keep.append(a)
            setattr(b, f, _ptr(a).value if a is not None else None)
        return b

    def depth_target(self, soa, tid, target_len, W, flag_mask=0x704, dev=False, runs_cap=None):
        """One chromosome of bam2depth: (runs[n,3] int32, win_sum uint64[target_len//W+1])."""
        keep = []
        self._ck(self.L.hpn_depth_begin(self.h, tid, target_len, flag_mask), "hpn_depth_begin")
        b = self._batch(soa, keep)
        add = self.L.hpn_depth_add_dev if dev else self.L.hpn_depth_add
        self._ck(add(self.h, C.byref(b)), "hpn_depth_add")
        return self.depth_finish(target_len, W, runs_cap)

    def depth_finish(self, target_len, W, runs_cap=None):
        win = np.zeros(target_len // W + 1, np.uint64)
        cap = runs_cap if runs_cap is not None else 1 << 16
        while True:
            runs = np.zeros((cap, 3), np.int32)
            nr = C.c_uint64(0)
            rc = self.L.hpn_depth_finish(self.h, W, _ptr(runs), cap, C.byref(nr), _ptr(win))
            if rc == _lib.E_CAPACITY:
                cap = int(nr.value)
                continue
            self._ck(rc, "hpn_depth_finish")
            return runs[:nr.value], win

    def depth_bedgraph_format(self, name):
        """Format the bedGraph text of the last depth_finish on the device; returns its size (the text stays there)."""
        nb = C.c_uint64(0)
        self._ck(self.L.hpn_depth_bedgraph_format(self.h, name.encode(), C.byref(nb)), "hpn_depth_bedgraph_format")
        return nb.value

    def depth_bedgraph(self, name):
        """bedGraph text of the runs of the last depth_finish, formatted on the device (read back in two pieces on purpose)."""
        nb = C.c_uint64(0)
        self._ck(self.L.hpn_depth_bedgraph_format(self.h, name.encode(), C.byref(nb)), "hpn_depth_bedgraph_format")
        out = np.zeros(max(nb.value, 1), np.uint8)
        cut = nb.value // 3
        self._ck(self.L.hpn_depth_bedgraph_read(self.h, 0, _ptr(out), cut), "hpn_depth_bedgraph_read")
        self._ck(self.L.hpn_depth_bedgraph_read(self.h, cut, out[cut:].ctypes.data, nb.value - cut), "hpn_depth_bedgraph_read")
        return out[:nb.value].tobytes()

    def window_counts(self, soa, win_off, W, dev=False):
        keep = []
        win_off = np.ascontiguousarray(win_off, np.uint64)
        nt = len(win_off) - 1
        self._ck(self.L.hpn_window_begin(self.h, nt, _ptr(win_off), W), "hpn_window_begin")
        b = self._batch(soa, keep)
        add = self.L.hpn_window_add_dev if dev else self.L.hpn_window_add
        self._ck(add(self.h, C.byref(b)), "hpn_window_add")
        tot = int(win_off[-1])
        bins, gc, ln = np.zeros(tot, np.uint32), np.zeros(tot, np.uint64), np.zeros(tot, np.uint32)
        touched = np.zeros(nt, np.uint8)
        nc = C.c_uint64(0)
        self._ck(self.L.hpn_window_finish(self.h, _ptr(bins), _ptr(gc), _ptr(ln), _ptr(touched), C.byref(nc)),
                 "hpn_window_finish")
        return bins, gc, ln, touched, nc.value

    # ---- BAM records in place in inflated BGZF blocks ------------------------------
    def bam_raw_index_dev(self, d_raw, d_blocks, n_blocks, first_off, d_status):
        info = _lib.RawInfo()
        self._ck(self.L.hpn_bam_raw_index_dev(self.h, _ptr(d_raw), _ptr(d_blocks), n_blocks, first_off, _ptr(d_status),
                                              C.byref(info)), "hpn_bam_raw_index_dev")
        return info

    def depth_target_raw(self, d_raw, tid, target_len, W, flag_mask=0x704):
        self._ck(self.L.hpn_depth_begin(self.h, tid, target_len, flag_mask), "hpn_depth_begin")
        self._ck(self.L.hpn_depth_add_raw_dev(self.h, _ptr(d_raw)), "hpn_depth_add_raw_dev")
        return self.depth_finish(target_len, W)

    def window_counts_raw(self, d_raw, win_off, W):
        win_off = np.ascontiguousarray(win_off, np.uint64)
        nt = len(win_off) - 1
        self._ck(self.L.hpn_window_begin(self.h, nt, _ptr(win_off), W), "hpn_window_begin")
        self._ck(self.L.hpn_window_add_raw_dev(self.h, _ptr(d_raw)), "hpn_window_add_raw_dev")
        tot = int(win_off[-1])
        bins, gc, ln = np.zeros(tot, np.uint32), np.zeros(tot, np.uint64), np.zeros(tot, np.uint32)
        touched = np.zeros(nt, np.uint8)
        nc = C.c_uint64(0)
        self._ck(self.L.hpn_window_finish(self.h, _ptr(bins), _ptr(gc), _ptr(ln), _ptr(touched), C.byref(nc)),
                 "hpn_window_finish")
        return bins, gc, ln, touched, nc.value

    # ---- bamSplitChr: target boundaries, domain checks, BGZF cuts (hpn_bam_split_*) ----
    def split_begin(self, n_ref, level0=False):
        self._ck(self.L.hpn_bam_split_begin(self.h, n_ref, 1 if level0 else 0), "hpn_bam_split_begin")

    def split_add_raw_dev(self, d_raw, last=False):
        """The batch hpn_bam_raw_index_dev indexed last (d_raw None: no records, only `last`) -> SplitInfo."""
        info = _lib.SplitInfo()
        self._ck(self.L.hpn_bam_split_add_raw_dev(self.h, _ptr(d_raw) if d_raw is not None else None, 1 if last else 0, C.byref(info)),
                 "hpn_bam_split_add_raw_dev")
        return info

    def split_blocks(self, n):
        """The n closed blocks of the last split_add_raw_dev -> ctypes array of SplitBlock (off, len, crc, tid)."""
        return self._last_blocks("hpn_bam_split_blocks", n)

    # what the record-store sessions (sort, rmdup, merge, fixmate) take and answer alike, by the C function's name
    def _raw_add(self, name, Info, d_raw):
        info = Info()
        self._ck(getattr(self.L, name)(self.h, _ptr(d_raw) if d_raw is not None else None, C.byref(info)), name)
        return info

    def _finish(self, name, Result):
        res = Result()
        self._ck(getattr(self.L, name)(self.h, C.byref(res)), name)
        return res

    def _order(self, name, n):
        out = np.zeros(int(n), np.uint32)
        self._ck(getattr(self.L, name)(self.h, _ptr(out) if n else None, int(n)), name)
        return out

    def _emit(self, name, first_record, max_records, last):
        info = _lib.SplitInfo()
        self._ck(getattr(self.L, name)(self.h, int(first_record), int(max_records), 1 if last else 0, C.byref(info)), name)
        return info

    # what the sessions that write BAM blocks (split and those four) answer alike, by the C function's name
    def _last_blocks(self, name, n):
        out = (_lib.SplitBlock * max(int(n), 1))()
        got = C.c_uint64(0)
        self._ck(getattr(self.L, name)(self.h, 0, out, int(n), C.byref(got)), name)
        return out[:got.value]

    def _dev_span(self, name):
        p, n = C.c_void_p(0), C.c_uint64(0)
        self._ck(getattr(self.L, name)(self.h, C.byref(p), C.byref(n)), name)
        return p.value or 0, n.value

    def _dev_span_bytes(self, name):
        p, n = self._dev_span(name)
        host = np.zeros(n, np.uint8)
        if n:
            self._ck(self.L.hpn_memcpy_d2h(self.h, _ptr(host), p, n), "hpn_memcpy_d2h")
            self.sync()
        return host.tobytes()

    def split_payload(self):
        """The payload buffer of the last call up to the end of its last closed block, copied to the host."""
        return self._dev_span_bytes("hpn_bam_split_payload_dev")

    def split_stored(self):
        """The closed blocks of the last call as the device framed them (level 0), copied to the host."""
        return self._dev_span_bytes("hpn_bam_split_stored_dev")

    def bgzf_stored_dev(self, d_data, spans, d_image):
        """spans: (off, img_off, len, crc) per block -> each framed as a stored BGZF block of len + 31 bytes at d_image + img_off."""
        arr = np.zeros(len(spans), np.dtype([("off", "<u8"), ("img_off", "<u8"), ("len", "<u4"), ("crc", "<u4")]))
        for k, sp in enumerate(spans):
            arr[k] = sp
        self._ck(self.L.hpn_bgzf_stored_dev(self.h, _ptr(d_data), _ptr(arr) if len(spans) else None, len(spans), _ptr(d_image)), "hpn_bgzf_stored_dev")

    def split_finish(self, n_ref):
        res, counts = _lib.SplitResult(), np.zeros(max(n_ref, 1), np.uint64)
        self._ck(self.L.hpn_bam_split_finish(self.h, C.byref(res), _ptr(counts)), "hpn_bam_split_finish")
        return res, counts[:n_ref]

    # ---- samtools index: the .bai of a coordinate-sorted BAM (hpn_bam_bai_*) ----
    BAI_TARGET = np.dtype([("off_beg", "<u8"), ("off_end", "<u8"), ("n_mapped", "<u8"), ("n_unmapped", "<u8"), ("first_chunk", "<u8"),
                           ("n_chunks", "<u8"), ("first_window", "<u8"), ("n_windows", "<i4"), ("has_records", "<u4")])
    BAI_CHUNK = np.dtype([("beg", "<u8"), ("end", "<u8"), ("bin", "<u4"), ("tid", "<i4")])

    def bam_bai_begin(self, target_len, first_voffset):
        """target_len: the header's target lengths; first_voffset: the virtual offset behind the header."""
        tl = np.ascontiguousarray(target_len, np.int32)
        self._ck(self.L.hpn_bam_bai_begin(self.h, len(tl), _ptr(tl) if len(tl) else None, int(first_voffset)), "hpn_bam_bai_begin")

    def bam_bai_add_raw_dev(self, d_raw, d_blocks=None, n_blocks=0, block_addr=(), last=False, end_voffset=0):
        """The batch hpn_bam_raw_index_dev indexed last with its block table and block_addr[0 .. n_blocks] = the blocks' file offsets
        and the offset behind the last (d_raw None: no records, only `last` with the file's final virtual offset) -> BaiInfo."""
        info = _lib.BaiInfo()
        addr = np.ascontiguousarray(block_addr, np.uint64)
        assert d_raw is None or len(addr) == n_blocks + 1
        self._ck(self.L.hpn_bam_bai_add_raw_dev(self.h, _ptr(d_raw) if d_raw is not None else None, _ptr(d_blocks) if d_blocks is not None else None,
                                                int(n_blocks), _ptr(addr) if len(addr) else None, 1 if last else 0, int(end_voffset), C.byref(info)),
                 "hpn_bam_bai_add_raw_dev")
        return info

    def bam_bai_finish(self):
        """-> (BaiResult, targets, chunks, windows): structured arrays of BAI_TARGET / BAI_CHUNK and the linear index's offsets."""
        res = _lib.BaiResult()
        self._ck(self.L.hpn_bam_bai_finish(self.h, C.byref(res)), "hpn_bam_bai_finish")
        targets, chunks = np.zeros(res.n_ref, self.BAI_TARGET), np.zeros(res.n_chunks, self.BAI_CHUNK)
        windows = np.zeros(res.n_windows, np.uint64)
        self._ck(self.L.hpn_bam_bai_read(self.h, _ptr(targets) if res.n_ref else None, _ptr(chunks) if res.n_chunks else None,
                                         _ptr(windows) if res.n_windows else None), "hpn_bam_bai_read")
        return res, targets, chunks, windows

    # ---- samtools sort: a BAM in coordinate order (hpn_bam_sort_*) ----
    def bam_sort_begin(self):
        self._ck(self.L.hpn_bam_sort_begin(self.h), "hpn_bam_sort_begin")

    def bam_sort_add_raw_dev(self, d_raw):
        """The batch hpn_bam_raw_index_dev indexed last goes into the session's record store (d_raw None: no records) -> BamSortInfo."""
        return self._raw_add("hpn_bam_sort_add_raw_dev", _lib.BamSortInfo, d_raw)

    def bam_sort_finish(self):
        """Sorts -> BamSortResult (n_records, payload_bytes, fresh_mem, the first record outside the domain, sort_bits)."""
        return self._finish("hpn_bam_sort_finish", _lib.BamSortResult)

    def bam_sort_order(self, n):
        """order[j]: the input ordinal of the j-th record of the output."""
        return self._order("hpn_bam_sort_order", n)

    def bam_sort_sizes(self, n):
        """sizes[i]: 4 + block_size of input record i."""
        out = np.zeros(int(n), np.uint32)
        self._ck(self.L.hpn_bam_sort_sizes(self.h, _ptr(out) if n else None, int(n)), "hpn_bam_sort_sizes")
        return out

    def bam_sort_emit(self, first_record, max_records, last=False):
        """The next slice of the sorted records: gathered, cut, every closed block with its CRC-32 -> SplitInfo."""
        return self._emit("hpn_bam_sort_emit", first_record, max_records, last)

    def bam_sort_blocks(self, n):
        """The n closed blocks of the last bam_sort_emit -> list of SplitBlock (off, len, crc, tid)."""
        return self._last_blocks("hpn_bam_sort_blocks", n)

    def bam_sort_payload(self):
        """The payload buffer of the last bam_sort_emit up to the end of its last closed block, copied to the host."""
        return self._dev_span_bytes("hpn_bam_sort_payload_dev")

    def bam_sort_payload_dev(self):
        """-> (device address, bytes) of the same, for callers that look at the buffer where it lies."""
        return self._dev_span("hpn_bam_sort_payload_dev")

    def bam_sort_stored(self):
        """The closed blocks of the last bam_sort_emit framed as stored BGZF blocks (level 0), copied to the host."""
        return self._dev_span_bytes("hpn_bam_sort_stored_dev")

    # ---- samtools rmdup: duplicates of a coordinate-sorted BAM removed (hpn_bam_rmdup_*) ----
    def bam_rmdup_begin(self, n_ref, ids=(), lib_of_id=(), n_libs=1):
        """ids: the header's @RG IDs (bytes), lib_of_id: each one's library in [1, n_libs); library 0: no RG, an unknown ID, no LB."""
        arr = (C.c_char_p * max(len(ids), 1))(*[bytes(i) for i in ids])
        lib = np.ascontiguousarray(lib_of_id, np.uint32)
        assert len(lib) == len(ids)
        self._ck(self.L.hpn_bam_rmdup_begin(self.h, int(n_ref), len(ids), C.cast(arr, C.c_void_p) if len(ids) else None, _ptr(lib) if len(ids) else None,
                                            int(n_libs)), "hpn_bam_rmdup_begin")
        self._rmdup_shape = (int(n_ref), int(n_libs))

    def bam_rmdup_add_raw_dev(self, d_raw):
        """The batch hpn_bam_raw_index_dev indexed last is classified and goes into the session's record store -> RmdupInfo."""
        return self._raw_add("hpn_bam_rmdup_add_raw_dev", _lib.RmdupInfo, d_raw)

    def bam_rmdup_finish(self):
        """Decides -> RmdupResult (n_records, n_out, payload_bytes, n_heads, the first record outside the domain)."""
        return self._finish("hpn_bam_rmdup_finish", _lib.RmdupResult)

    def bam_rmdup_counts(self):
        """-> ([(checked, removed, first head's ordinal or -1)] per library, [(has records, unmatched names)] per target and, last,
        for the unplaced records behind them)"""
        n_ref, n_libs = self._rmdup_shape
        libs, targets = (_lib.RmdupLib * n_libs)(), (_lib.RmdupTarget * (n_ref + 1))()
        self._ck(self.L.hpn_bam_rmdup_counts(self.h, C.cast(libs, C.c_void_p), C.cast(targets, C.c_void_p)), "hpn_bam_rmdup_counts")
        return [(l.checked, l.removed, l.first) for l in libs], [(bool(t.has_records), t.unmatched) for t in targets]

    def bam_rmdup_order(self, n):
        """order[j]: the input ordinal of the j-th record of the output."""
        return self._order("hpn_bam_rmdup_order", n)

    def bam_rmdup_emit(self, first_record, max_records, last=False):
        """The next slice of the surviving records: gathered, cut, every closed block with its CRC-32 -> SplitInfo."""
        return self._emit("hpn_bam_rmdup_emit", first_record, max_records, last)

    def bam_rmdup_blocks(self, n):
        """The n closed blocks of the last bam_rmdup_emit -> list of SplitBlock (off, len, crc, tid)."""
        return self._last_blocks("hpn_bam_rmdup_blocks", n)

    def bam_rmdup_payload(self):
        """The payload buffer of the last bam_rmdup_emit up to the end of its last closed block, copied to the host."""
        return self._dev_span_bytes("hpn_bam_rmdup_payload_dev")

    def bam_rmdup_payload_dev(self):
        """-> (device address, bytes) of the same, for callers that look at the buffer where it lies."""
        return self._dev_span("hpn_bam_rmdup_payload_dev")

    def bam_rmdup_stored(self):
        """The closed blocks of the last bam_rmdup_emit framed as stored BGZF blocks (level 0), copied to the host."""
        return self._dev_span_bytes("hpn_bam_rmdup_stored_dev")

    # ---- samtools merge: several BAMs merged into one (hpn_bam_merge_*) ----
    def bam_merge_begin(self):
        self._ck(self.L.hpn_bam_merge_begin(self.h), "hpn_bam_merge_begin")

    def bam_merge_next_file(self):
        """The batches that follow belong to the next input file (a file of no batches is legal)."""
        self._ck(self.L.hpn_bam_merge_next_file(self.h), "hpn_bam_merge_next_file")

    def bam_merge_add_raw_dev(self, d_raw):
        """The batch hpn_bam_raw_index_dev indexed last goes into the session's record store (d_raw None: no records) -> BamMergeInfo."""
        return self._raw_add("hpn_bam_merge_add_raw_dev", _lib.BamMergeInfo, d_raw)

    def bam_merge_finish(self):
        """Merges -> BamMergeResult (n_records, n_files, payload_bytes, n_lifted, the first record outside the domain, sort_bits)."""
        return self._finish("hpn_bam_merge_finish", _lib.BamMergeResult)

    def bam_merge_order(self, n):
        """order[j]: the session ordinal of the j-th record of the output."""
        return self._order("hpn_bam_merge_order", n)

    def bam_merge_emit(self, first_record, max_records, last=False):
        """The next slice of the merged records: gathered, cut, every closed block with its CRC-32 -> SplitInfo."""
        return self._emit("hpn_bam_merge_emit", first_record, max_records, last)

    def bam_merge_blocks(self, n):
        """The n closed blocks of the last bam_merge_emit -> list of SplitBlock (off, len, crc, tid)."""
        return self._last_blocks("hpn_bam_merge_blocks", n)

    def bam_merge_payload(self):
        """The payload buffer of the last bam_merge_emit up to the end of its last closed block, copied to the host."""
        return self._dev_span_bytes("hpn_bam_merge_payload_dev")

    def bam_merge_stored(self):
        """The closed blocks of the last bam_merge_emit framed as stored BGZF blocks (level 0), copied to the host."""
        return self._dev_span_bytes("hpn_bam_merge_stored_dev")

    # ---- samtools fixmate: mate fields of a name-grouped BAM filled in (hpn_bam_fixmate_*) ----
    def bam_fixmate_begin(self, remove_reads, target_len):
        """target_len: the header's l_ref values; remove_reads: -r, records without a refID and secondary ones are dropped."""
        tl = np.ascontiguousarray(target_len, dtype=np.uint32)
        self._ck(self.L.hpn_bam_fixmate_begin(self.h, 1 if remove_reads else 0, int(tl.size), _ptr(tl) if tl.size else None), "hpn_bam_fixmate_begin")

    def bam_fixmate_add_raw_dev(self, d_raw):
        """The batch hpn_bam_raw_index_dev indexed last goes into the session's record store (d_raw None: no records) -> FixmateInfo."""
        return self._raw_add("hpn_bam_fixmate_add_raw_dev", _lib.FixmateInfo, d_raw)

    def bam_fixmate_finish(self):
        """Decides -> FixmateResult (records in and out, pairs, singletons, CT fields, bytes added, the first record outside the domain)."""
        return self._finish("hpn_bam_fixmate_finish", _lib.FixmateResult)

    def bam_fixmate_order(self, n):
        """order[j]: the session ordinal of the j-th record of the output."""
        return self._order("hpn_bam_fixmate_order", n)

    def bam_fixmate_emit(self, first_record, max_records, last=False):
        """The next slice of the output: gathered, rewritten, cut, every closed block with its CRC-32 -> SplitInfo."""
        return self._emit("hpn_bam_fixmate_emit", first_record, max_records, last)

    def bam_fixmate_blocks(self, n):
        """The n closed blocks of the last bam_fixmate_emit -> list of SplitBlock (off, len, crc, tid)."""
        return self._last_blocks("hpn_bam_fixmate_blocks", n)

    def bam_fixmate_payload(self):
        """The payload buffer of the last bam_fixmate_emit up to the end of its last closed block, copied to the host."""
        return self._dev_span_bytes("hpn_bam_fixmate_payload_dev")

    def bam_fixmate_stored(self):
        """The closed blocks of the last bam_fixmate_emit framed as stored BGZF blocks (level 0), copied to the host."""
        return self._dev_span_bytes("hpn_bam_fixmate_stored_dev")

    # ---- samtools view: a BAM's records filtered, as BAM, as SAM text or counted (hpn_bam_view_*) ----
    VIEW_BAM, VIEW_TEXT, VIEW_COUNT = 0, 1, 2

    def bam_view_begin(self, emit, flag_on=0, flag_off=0, min_mapq=0, min_qlen=0, qual_scale=0, subsample=False, seed=0, threshold=0, flag_style=0,
                       target_names=(), rg_id=None, rg_ids=None, lib_ids=None):
        """Opens a session.  emit: VIEW_BAM, VIEW_TEXT or VIEW_COUNT; threshold: ceil(fraction * 2^24) of -s; target_names: the
        header's names as bytes, for text.  The read-group rule, as bytes: rg_id (-r), rg_ids (-R: a list, empty too), lib_ids (-l:
        the IDs whose LB is the library, empty too); None: not given."""
        names = b"".join(target_names)
        off = np.zeros(len(target_names) + 1, np.uint32)
        off[1:] = np.cumsum([len(n) for n in target_names], dtype=np.uint64)
        buf = np.frombuffer(names + b"\0", np.uint8).copy()
        o = _lib.ViewOpts(flag_on, flag_off, min_mapq, min_qlen, qual_scale, 1 if subsample else 0, seed, threshold, emit, flag_style, len(target_names), 0,
                          buf.ctypes.data, off.ctypes.data)
        strings = lambda ids: (C.c_char_p * max(len(ids), 1))(*ids)
        o.rg_id = rg_id
        if rg_ids is not None:
            o.rg_ids, o.n_rg_ids, o.has_rg_ids = strings(list(rg_ids)), len(rg_ids), 1
        if lib_ids is not None:
            o.lib_ids, o.n_lib_ids, o.has_library = strings(list(lib_ids)), len(lib_ids), 1
        self._ck(self.L.hpn_bam_view_begin(self.h, C.byref(o)), "hpn_bam_view_begin")

    def bam_view_add_raw_dev(self, d_raw):
        """The batch hpn_bam_raw_index_dev indexed last is classified and goes into the session's record store -> ViewInfo."""
        return self._raw_add("hpn_bam_view_add_raw_dev", _lib.ViewInfo, d_raw)

    def bam_view_finish(self):
        """Decides -> ViewResult (records in, records kept -- the count --, their bytes as BAM or as text, the first record outside the domain)."""
        return self._finish("hpn_bam_view_finish", _lib.ViewResult)

    def bam_view_order(self, n):
        """order[j]: the session ordinal of the j-th kept record (n = ViewResult.n_out)."""
        return self._order("hpn_bam_view_order", n)

    def bam_view_emit(self, first_record, max_records, last=False):
        """The next slice of a VIEW_BAM session's output, cut into blocks with their CRC-32 -> SplitInfo."""
        return self._emit("hpn_bam_view_emit", first_record, max_records, last)

    def bam_view_blocks(self, n):
        """The n closed blocks of the last bam_view_emit -> list of SplitBlock (off, len, crc, tid)."""
        return self._last_blocks("hpn_bam_view_blocks", n)

    def bam_view_payload(self):
        """The payload buffer of the last bam_view_emit up to the end of its last closed block, copied to the host."""
        return self._dev_span_bytes("hpn_bam_view_payload_dev")

    def bam_view_stored(self):
        """The closed blocks of the last bam_view_emit framed as stored BGZF blocks (level 0), copied to the host."""
        return self._dev_span_bytes("hpn_bam_view_stored_dev")

    def bam_view_text(self, first_record, max_records):
        """The next slice of a VIEW_TEXT session's lines -> (ViewTextInfo, the lines' bytes copied to the host)."""
        info = _lib.ViewTextInfo()
        self._ck(self.L.hpn_bam_view_text_emit(self.h, int(first_record), int(max_records), C.byref(info)), "hpn_bam_view_text_emit")
        return info, self._dev_span_bytes("hpn_bam_view_text_dev")

    # ---- collectives / synthetic -----------------------------------------
    def comm_init(self, rank, n_ranks, unique_id: bytes):
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._ck(self.L.hpn_comm_init(self.h, rank, n_ranks, buf), "hpn_comm_init")

    def allreduce_u64(self, d_vec, n):
        self._ck(self.L.hpn_allreduce_u64(self.h, _ptr(d_vec), n), "hpn_allreduce_u64")

    def comm_count(self) -> int:
        """Ranks of this context's communicator as RCCL reports them (ncclCommCount)."""
        n = C.c_int(0)
        self._ck(self.L.hpn_comm_count(self.h, C.byref(n)), "hpn_comm_count")
        return n.value

    def synth_fastq_dev(self, seed, first, n, length, d_qual, d_base, d_off):
        self._ck(self.L.hpn_synth_fastq_dev(self.h, seed, first, n, length, _ptr(d_qual), _ptr(d_base), _ptr(d_off)),
                 "hpn_synth_fastq_dev")


def comm_init_all(ctxs):
    """One communicator per context of THIS process (ncclCommInitAll): the contexts must sit on distinct devices."""
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    rc = _lib.lib().hpn_comm_init_all(arr, len(ctxs))
    if rc != 0:
        raise HpnError(rc, "hpn_comm_init_all", _lib.lib().hpn_ctx_last_error(ctxs[0].h).decode() if ctxs else "")


def allreduce_u64_all(ctxs, d_vecs, n_words):
    """Sum d_vecs[i] (on ctxs[i]'s device) in place into every one of them, in one RCCL group."""
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    vec = (C.c_void_p * len(ctxs))(*[v if isinstance(v, int) else _ptr(v) for v in d_vecs])
    rc = _lib.lib().hpn_allreduce_u64_all(arr, vec, len(ctxs), n_words)
    if rc != 0:
        raise HpnError(rc, "hpn_allreduce_u64_all", _lib.lib().hpn_ctx_last_error(ctxs[0].h).decode() if ctxs else "")


def comm_library() -> str:
    """Path of the RCCL library the binding resolved to ('' before the first use / when none could be loaded)."""
    return _lib.lib().hpn_comm_library().decode()


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES)()
    rc = _lib.lib().hpn_comm_unique_id(buf)
    if rc != 0:
        raise HpnError(rc, "hpn_comm_unique_id")
    return bytes(buf)


def device_count() -> int:
    n = C.c_int(0)
    _lib.lib().hpn_device_count(C.byref(n))
    return n.value
