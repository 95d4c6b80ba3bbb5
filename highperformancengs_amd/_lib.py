"""ctypes binding of libhpngs.so (the C ABI in include/hpngs.h).

There is no fallback: if the library is missing or a call fails, this raises.
Inside a PyTorch process import torch BEFORE this module so that both share the
one libamdhip64.so.7 / librccl.so.1 torch ships (same sonames as /opt/rocm).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HPN_LIB") or os.path.join(HERE, "libhpngs.so")   # HPN_LIB: A/B runs of a variant build

LEN_BINS, QUAL_ROWS, NUC_CODES = 512, 128, 5
W_SEQLEN, W_TOTAL, W_Q20, W_Q30, W_BAD, W_QUAL = 0, 512, 513, 514, 515, 516
W_NUC = W_QUAL + QUAL_ROWS * LEN_BINS
TALLY_WORDS = W_NUC + NUC_CODES * LEN_BINS
TALLY_QUAL_HIST, TALLY_NUC_HIST = 1, 2
DEPTH_ANY_ORDER = 0x80000000
UNIQUE_ID_BYTES = 128

OK, E_NODEVICE, E_HIP, E_ARG, E_DOMAIN, E_NOMEM, E_STATE, E_RCCL, E_CAPACITY, E_PARTIAL = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9


class HpnError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: status {status} ({_strerror(status)}) {detail}".strip())


class Tally(C.Structure):
    _fields_ = [("seqlen", C.c_uint64 * LEN_BINS), ("total", C.c_uint64), ("q20", C.c_uint64),
                ("q30", C.c_uint64), ("qual_hist", C.POINTER(C.c_uint64)), ("nuc_hist", C.POINTER(C.c_uint64))]


class TextInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_bytes", C.c_uint64), ("carry_bytes", C.c_uint64),
                ("irregular", C.c_uint32), ("reserved", C.c_uint32)]


class SampleRule(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("fasta", C.c_uint32), ("seed_add", C.c_uint32), ("threshold", C.c_uint32),
                ("picks", C.c_void_p), ("n_picks", C.c_uint64), ("first_ordinal", C.c_uint64)]


class SampleInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_kept", C.c_uint64), ("n_bytes", C.c_uint64), ("carry_bytes", C.c_uint64),
                ("irregular", C.c_uint32), ("reserved", C.c_uint32)]


SAMPLE_FRACTION, SAMPLE_PICKS = 1, 2


class UniqInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("irregular", C.c_uint32), ("reserved", C.c_uint32)]


class UniqResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unique", C.c_uint64), ("hash_size", C.c_uint64), ("unmatched", C.c_int64),
                ("out_bytes", C.c_uint64 * 2), ("hash_clashes", C.c_uint64), ("unmatched_name", C.c_char * 1024)]


UNIQ_TABLE_ORDER, UNIQ_KEY_ORDER = 0, 1


class UniqqResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unique", C.c_uint64), ("hash_size", C.c_uint64), ("hash_clashes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("max_count", C.c_uint32), ("reserved", C.c_uint32)]


UNIQQ_KEY_ORDER, UNIQQ_COUNT_ORDER = 0, 1


class UsortResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unique", C.c_uint64), ("table_reads", C.c_uint64), ("hash_size", C.c_uint64),
                ("unmatched", C.c_int64), ("out_bytes", C.c_uint64 * 2), ("hash_clashes", C.c_uint64), ("max_count", C.c_uint32),
                ("seq_len", C.c_uint32), ("no_answer", C.c_uint32), ("reserved", C.c_uint32), ("unmatched_name", C.c_char * 1024)]


USORT_FEW_READS, USORT_LONG_KEY, USORT_SHORT_KEY = 1, 2, 3


class SortInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("irregular", C.c_uint32), ("reserved", C.c_uint32)]


class SortResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("out_bytes", C.c_uint64), ("refined", C.c_uint64), ("rounds", C.c_uint32), ("lone_line", C.c_uint32)]


class KseqResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_distinct", C.c_uint64), ("out_bytes", C.c_uint64), ("refined", C.c_uint64), ("rounds", C.c_uint32),
                ("shape", C.c_uint32), ("one_length", C.c_uint32), ("first_len", C.c_uint32), ("other_len", C.c_uint32), ("reserved", C.c_uint32)]


KSEQ_NONE, KSEQ_FASTA, KSEQ_FASTQ = 0, 1, 2


class TwobitResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("out_bytes", C.c_uint64), ("bad_record", C.c_int64), ("seq_len", C.c_uint32), ("packed_len", C.c_uint32)]


class PairResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64 * 2), ("n_pairs", C.c_uint64), ("n_single", C.c_uint64 * 2), ("out_bytes", C.c_uint64 * 4),
                ("fail_record", C.c_int64), ("fail_mate", C.c_uint32), ("route", C.c_uint32), ("unverified", C.c_uint32), ("reserved", C.c_uint32)]


class MrleResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("out_bytes", C.c_uint64 * 3), ("bad_record", C.c_int64)]


MRLE_PACKED, MRLE_TEXT, MRLE_SHARED = 0, 1, 2


class RfastqcResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unique", C.c_uint64), ("hash_clashes", C.c_uint64), ("bad_record", C.c_int64),
                ("bad_mate", C.c_uint32), ("reason", C.c_uint32)]


RFASTQC_DUP, RFASTQC_GC, RFASTQC_QUALITY, RFASTQC_NUCLEOTIDE, RFASTQC_LENGTH = 0, 1, 2, 3, 4
RFASTQC_BAD_LENGTH, RFASTQC_BAD_QUALITY, RFASTQC_BAD_BYTE, RFASTQC_MATE_SHORT = 1, 2, 3, 4


class TextPiece(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("irregular", C.c_uint32), ("reserved", C.c_uint32)]


TEXT_PIECE_TAIL = 4096
TEXT_NUL, TEXT_LONG_LINE, TEXT_RAGGED, TEXT_PARTIAL, TEXT_LEN, TEXT_DENSE, TEXT_STALE = 1, 2, 4, 8, 16, 32, 64
TEXT_SHORT_QUAL = 128
TEXT_KSEQ = 256
TEXT_INPLACE_PAD = 8192


class Rqc(C.Structure):
    _fields_ = [("quality", C.POINTER(C.c_int32)), ("nucleotide", C.POINTER(C.c_int32)), ("length", C.POINTER(C.c_int32)),
                ("gc", C.POINTER(C.c_double))]


RQC_MAXLEN = 300


class RawInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("tid_min", C.c_int32), ("tid_max", C.c_int32), ("flags", C.c_uint32),
                ("tail_bytes", C.c_uint32)]


class SplitInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_blocks", C.c_uint64), ("payload_bytes", C.c_uint64), ("stored_bytes", C.c_uint64),
                ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32), ("tid_first", C.c_int32), ("tid_last", C.c_int32),
                ("reason", C.c_uint32), ("open_bytes", C.c_uint32)]


class SplitBlock(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("crc", C.c_uint32), ("tid", C.c_int32), ("reserved", C.c_uint32)]


class SplitResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_blocks", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("n_ref", C.c_uint32)]


class BaiInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_runs", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class BaiResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_chunks", C.c_uint64), ("n_windows", C.c_uint64), ("n_no_coor", C.c_uint64), ("bad_record", C.c_int64),
                ("bad_tid", C.c_int32), ("bad_pos", C.c_int32), ("reason", C.c_uint32), ("n_ref", C.c_uint32)]


class BamSortInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class BamSortResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("payload_bytes", C.c_uint64), ("fresh_mem", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32),
                ("bad_pos", C.c_int32), ("reason", C.c_uint32), ("sort_bits", C.c_uint32)]


class BamMergeInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class BamMergeResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_files", C.c_uint64), ("payload_bytes", C.c_uint64), ("n_lifted", C.c_uint64), ("bad_record", C.c_int64),
                ("bad_tid", C.c_int32), ("bad_pos", C.c_int32), ("reason", C.c_uint32), ("sort_bits", C.c_uint32)]


class FixmateInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class FixmateResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_out", C.c_uint64), ("n_pairs", C.c_uint64), ("n_singletons", C.c_uint64), ("n_tags", C.c_uint64),
                ("bytes_added", C.c_uint64), ("payload_bytes", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class ViewOpts(C.Structure):
    _fields_ = [("flag_on", C.c_uint32), ("flag_off", C.c_uint32), ("min_mapq", C.c_uint32), ("min_qlen", C.c_int32), ("qual_scale", C.c_int32),
                ("subsample", C.c_uint32), ("seed", C.c_uint32), ("threshold", C.c_uint32), ("emit", C.c_uint32), ("flag_style", C.c_uint32),
                ("n_targets", C.c_int32), ("reserved", C.c_uint32), ("target_names", C.c_void_p), ("target_name_off", C.c_void_p),
                ("rg_id", C.c_char_p), ("rg_ids", C.POINTER(C.c_char_p)), ("lib_ids", C.POINTER(C.c_char_p)), ("n_rg_ids", C.c_uint32),
                ("n_lib_ids", C.c_uint32), ("has_rg_ids", C.c_uint32), ("has_library", C.c_uint32), ("reserved2", C.c_uint64 * 4)]


class ViewInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class ViewResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_out", C.c_uint64), ("payload_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("bad_record", C.c_int64),
                ("bad_tid", C.c_int32), ("bad_pos", C.c_int32), ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class ViewTextInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_bytes", C.c_uint64)]


class RmdupInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("store_bytes", C.c_uint64), ("bad_record", C.c_int64), ("bad_tid", C.c_int32), ("bad_pos", C.c_int32),
                ("reason", C.c_uint32), ("reserved", C.c_uint32)]


class RmdupResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_out", C.c_uint64), ("payload_bytes", C.c_uint64), ("n_heads", C.c_uint64), ("bad_record", C.c_int64),
                ("bad_tid", C.c_int32), ("bad_pos", C.c_int32), ("reason", C.c_uint32), ("n_libs", C.c_uint32), ("n_ref", C.c_uint32), ("reserved", C.c_uint32)]


class RmdupLib(C.Structure):
    _fields_ = [("checked", C.c_uint64), ("removed", C.c_uint64), ("first", C.c_int64)]


class RmdupTarget(C.Structure):
    _fields_ = [("unmatched", C.c_uint64), ("has_records", C.c_uint32), ("reserved", C.c_uint32)]


class GzInfo(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("end_bit", C.c_uint64), ("status", C.c_uint32), ("bad_chunk", C.c_uint32),
                ("final_chunk", C.c_uint32), ("reserved", C.c_uint32)]


class Run(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("depth", C.c_int32)]


class BamBatch(C.Structure):
    _fields_ = [("n", C.c_uint64), ("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p),
                ("l_qseq", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq4", C.c_void_p)]


# every symbol include/hpngs.h declares: (name, restype, argtypes)
_vp, _u64, _u32, _i32, _int, _sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int, C.c_size_t
SYMBOLS = [
    ("hpn_abi_version", _int, []),
    ("hpn_strerror", C.c_char_p, [_int]),
    ("hpn_device_count", _int, [C.POINTER(_int)]),
    ("hpn_ctx_create", _int, [_int, C.POINTER(_vp)]),
    ("hpn_ctx_destroy", _int, [_vp]),
    ("hpn_ctx_set_stream", _int, [_vp, _vp]),
    ("hpn_ctx_sync", _int, [_vp]),
    ("hpn_ctx_device", _int, [_vp, C.POINTER(C.c_int)]),
    ("hpn_ctx_pci_address", _int, [_vp, C.c_char_p, _int]),
    ("hpn_ctx_last_error", C.c_char_p, [_vp]),
    ("hpn_ctx_last_kernel_ms", _int, [_vp, _int, C.POINTER(C.c_float)]),
    ("hpn_dev_malloc", _int, [_vp, _sz, C.POINTER(_vp)]),
    ("hpn_dev_mem_info", _int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("hpn_dev_free", _int, [_vp, _vp]),
    ("hpn_host_malloc", _int, [_vp, _sz, C.POINTER(_vp)]),
    ("hpn_host_free", _int, [_vp, _vp]),
    ("hpn_memcpy_h2d", _int, [_vp, _vp, _vp, _sz]),
    ("hpn_memcpy_d2h", _int, [_vp, _vp, _vp, _sz]),
    ("hpn_memcpy_d2d", _int, [_vp, _vp, _vp, _sz]),
    ("hpn_fastq_tally", _int, [_vp, _vp, _vp, _vp, _u64, C.POINTER(Tally)]),
    ("hpn_fastq_tally_dev", _int, [_vp, _vp, _vp, _vp, _u64, _u32]),
    ("hpn_fastq_tally_fetch", _int, [_vp, C.POINTER(Tally)]),
    ("hpn_fastq_tally_devptr", _int, [_vp, C.POINTER(_vp)]),
    ("hpn_fastq_rqc", _int, [_vp, _vp, _vp, _vp, _u64, C.POINTER(Rqc)]),
    ("hpn_fastq_read_gc_dev", _int, [_vp, _vp, _vp, _u64, _vp]),
    ("hpn_fastq_trim", _int, [_vp, _vp, _vp, _vp, _u64, _i32, _i32, _vp, _vp, _vp]),
    ("hpn_fastq_trim_dev", _int, [_vp, _vp, _vp, _vp, _u64, _i32, _i32, _vp, _vp, _vp]),
    ("hpn_fastq_qtrim_points", _int, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    ("hpn_fastq_qtrim_points_dev", _int, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    ("hpn_fastq_trim_points", _int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("hpn_fastq_trim_points_dev", _int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("hpn_fastq_text_begin", _int, [_vp]),
    ("hpn_fastq_text_count", _int, [_vp, _vp, _u64, _int, _u32, C.POINTER(TextInfo)]),
    ("hpn_fastq_text_count_inplace", _int, [_vp, _vp, _u64, _int, _u32, C.POINTER(TextInfo)]),
    ("hpn_fastq_text_records", _int, [_vp, _vp, _u64, _int, C.POINTER(TextInfo)]),
    ("hpn_fastq_text_trim", _int, [_vp, _vp, _u64, _int, _i32, _i32, _vp, _u64, C.POINTER(TextInfo)]),
    ("hpn_fastq_text_sample", _int, [_vp, _vp, _u64, _int, C.POINTER(SampleRule), _vp, _u64, _vp, _u64, C.POINTER(SampleInfo)]),
    ("hpn_fastq_uniq_begin", _int, [_vp, _int, _u64, _u32]),
    ("hpn_fastq_uniq_add", _int, [_vp, _int, _vp, _u64, _int, C.POINTER(UniqInfo)]),
    ("hpn_fastq_uniq_finish", _int, [_vp, C.POINTER(UniqResult)]),
    ("hpn_fastq_uniq_write", _int, [_vp, _int, _int, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_sort_pairs_u64", _int, [_vp, _vp, _vp, _u64]),
    ("hpn_sort_pairs_u64_bits", _int, [_vp, _vp, _vp, _u64, _int, _int]),
    ("hpn_sort_pairs_u64_digits", _int, [_vp, _vp, _vp, _u64, _u32]),
    ("hpn_excl_scan", _int, [_vp, _vp, _int, _vp, _int, _u64]),
    ("hpn_fastq_uniqq_begin", _int, [_vp, _u64, _u32]),
    ("hpn_fastq_uniqq_add", _int, [_vp, _vp, _u64, _int, C.POINTER(UniqInfo)]),
    ("hpn_fastq_uniqq_finish", _int, [_vp, C.POINTER(UniqqResult)]),
    ("hpn_fastq_uniqq_write", _int, [_vp, _int, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_fastq_usort_begin", _int, [_vp, _int, _u64, _u32]),
    ("hpn_fastq_usort_add", _int, [_vp, _int, _vp, _u64, _int, C.POINTER(UniqInfo)]),
    ("hpn_fastq_usort_finish", _int, [_vp, C.POINTER(UsortResult)]),
    ("hpn_fastq_usort_write", _int, [_vp, _int, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_fastq_sort_begin", _int, [_vp, _int, _u64]),
    ("hpn_fastq_sort_add", _int, [_vp, _vp, _u64, _int, C.POINTER(SortInfo)]),
    ("hpn_fastq_sort_finish", _int, [_vp, C.POINTER(SortResult)]),
    ("hpn_fastq_sort_write", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_kseq_begin", _int, [_vp, _u64]),
    ("hpn_kseq_add", _int, [_vp, _vp, _u64, _int, C.POINTER(SortInfo)]),
    ("hpn_kseq_finish", _int, [_vp, C.POINTER(KseqResult)]),
    ("hpn_kseq_write", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_twobit_pack_begin", _int, [_vp, _u64]),
    ("hpn_twobit_pack_add", _int, [_vp, _vp, _u64, _int, C.POINTER(SortInfo)]),
    ("hpn_twobit_pack_finish", _int, [_vp, C.POINTER(TwobitResult)]),
    ("hpn_twobit_pack_write", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_twobit_unpack", _int, [_vp, _u32, _u32, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_fastq_pair_begin", _int, [_vp, _u64]),
    ("hpn_fastq_pair_add", _int, [_vp, _int, _vp, _u64, _int, C.POINTER(SortInfo)]),
    ("hpn_fastq_pair_finish", _int, [_vp, C.POINTER(PairResult)]),
    ("hpn_fastq_pair_write", _int, [_vp, _int, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_mrle_begin", _int, [_vp, _u64]),
    ("hpn_mrle_add", _int, [_vp, _vp, _u64, _int, C.POINTER(SortInfo)]),
    ("hpn_mrle_finish", _int, [_vp, C.POINTER(MrleResult)]),
    ("hpn_mrle_write", _int, [_vp, _int, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_rfastqc_begin", _int, [_vp, _int, _u64, _u32]),
    ("hpn_rfastqc_add", _int, [_vp, _int, _vp, _u64, _int, C.POINTER(SortInfo)]),
    ("hpn_rfastqc_finish", _int, [_vp, C.POINTER(RfastqcResult)]),
    ("hpn_rfastqc_read", _int, [_vp, _int, _int, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_fastq_text_piece_lines", _int, [_vp, _vp, _u64, _u32, _u64, _int, C.POINTER(TextPiece)]),
    ("hpn_fastq_text_piece_count", _int, [_vp, _u64, _u32, C.POINTER(TextInfo)]),
    ("hpn_fastq_text_piece_trim", _int, [_vp, _u64, _i32, _i32, _vp, _u64, C.POINTER(TextInfo)]),
    ("hpn_bgzf_inflate_dev", _int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("hpn_gz_inflate_dev", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _u64, _vp, C.POINTER(GzInfo)]),
    ("hpn_inflate_slots", _int, [_vp, C.POINTER(_u32)]),
    ("hpn_gz_inflate_begin_dev", _int, [_vp, _vp, _vp, _u32, _u32]),
    ("hpn_gz_inflate_finish_dev", _int, [_vp, _vp, _vp, _u64, _vp, C.POINTER(GzInfo)]),
    ("hpn_gz_members", _int, [_vp, _vp, _u32, C.POINTER(_u32)]),
    ("hpn_crc32_dev", _int, [_vp, _vp, _vp, _u32, _vp]),
    ("hpn_gz_find_starts_dev", _int, [_vp, _vp, C.c_uint64, _vp, _u32, _vp]),
    ("hpn_crc32_join", _u32, [_u32, _u32, _u64]),
    ("hpn_bam_raw_index_dev", _int, [_vp, _vp, _vp, _u64, _u32, _vp, C.POINTER(RawInfo)]),
    ("hpn_depth_add_raw_dev", _int, [_vp, _vp]),
    ("hpn_window_add_raw_dev", _int, [_vp, _vp]),
    ("hpn_bgzf_stored_dev", _int, [_vp, _vp, _vp, _u32, _vp]),
    ("hpn_bam_split_begin", _int, [_vp, _i32, _int]),
    ("hpn_bam_split_add_raw_dev", _int, [_vp, _vp, _int, C.POINTER(SplitInfo)]),
    ("hpn_bam_split_blocks", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_bam_split_payload_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_split_stored_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_split_finish", _int, [_vp, C.POINTER(SplitResult), _vp]),
    ("hpn_bam_bai_begin", _int, [_vp, _i32, _vp, _u64]),
    ("hpn_bam_bai_add_raw_dev", _int, [_vp, _vp, _vp, _u64, _vp, _int, _u64, C.POINTER(BaiInfo)]),
    ("hpn_bam_bai_finish", _int, [_vp, C.POINTER(BaiResult)]),
    ("hpn_bam_bai_read", _int, [_vp, _vp, _vp, _vp]),
    ("hpn_bam_sort_begin", _int, [_vp]),
    ("hpn_bam_sort_add_raw_dev", _int, [_vp, _vp, C.POINTER(BamSortInfo)]),
    ("hpn_bam_sort_finish", _int, [_vp, C.POINTER(BamSortResult)]),
    ("hpn_bam_sort_order", _int, [_vp, _vp, _u64]),
    ("hpn_bam_sort_sizes", _int, [_vp, _vp, _u64]),
    ("hpn_bam_sort_emit", _int, [_vp, _u64, _u64, _int, C.POINTER(SplitInfo)]),
    ("hpn_bam_sort_blocks", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_bam_sort_payload_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_sort_stored_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_merge_begin", _int, [_vp]),
    ("hpn_bam_merge_next_file", _int, [_vp]),
    ("hpn_bam_merge_add_raw_dev", _int, [_vp, _vp, C.POINTER(BamMergeInfo)]),
    ("hpn_bam_merge_finish", _int, [_vp, C.POINTER(BamMergeResult)]),
    ("hpn_bam_merge_order", _int, [_vp, _vp, _u64]),
    ("hpn_bam_merge_emit", _int, [_vp, _u64, _u64, _int, C.POINTER(SplitInfo)]),
    ("hpn_bam_merge_blocks", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_bam_merge_payload_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_merge_stored_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_fixmate_begin", _int, [_vp, _int, _i32, _vp]),
    ("hpn_bam_fixmate_add_raw_dev", _int, [_vp, _vp, C.POINTER(FixmateInfo)]),
    ("hpn_bam_fixmate_finish", _int, [_vp, C.POINTER(FixmateResult)]),
    ("hpn_bam_fixmate_order", _int, [_vp, _vp, _u64]),
    ("hpn_bam_fixmate_emit", _int, [_vp, _u64, _u64, _int, C.POINTER(SplitInfo)]),
    ("hpn_bam_fixmate_blocks", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_bam_fixmate_payload_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_fixmate_stored_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_view_begin", _int, [_vp, C.POINTER(ViewOpts)]),
    ("hpn_bam_view_add_raw_dev", _int, [_vp, _vp, C.POINTER(ViewInfo)]),
    ("hpn_bam_view_finish", _int, [_vp, C.POINTER(ViewResult)]),
    ("hpn_bam_view_order", _int, [_vp, _vp, _u64]),
    ("hpn_bam_view_emit", _int, [_vp, _u64, _u64, _int, C.POINTER(SplitInfo)]),
    ("hpn_bam_view_blocks", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_bam_view_payload_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_view_stored_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_view_text_emit", _int, [_vp, _u64, _u64, C.POINTER(ViewTextInfo)]),
    ("hpn_bam_view_text_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_rmdup_begin", _int, [_vp, _i32, _u32, _vp, _vp, _u32]),
    ("hpn_bam_rmdup_add_raw_dev", _int, [_vp, _vp, C.POINTER(RmdupInfo)]),
    ("hpn_bam_rmdup_finish", _int, [_vp, C.POINTER(RmdupResult)]),
    ("hpn_bam_rmdup_counts", _int, [_vp, _vp, _vp]),
    ("hpn_bam_rmdup_order", _int, [_vp, _vp, _u64]),
    ("hpn_bam_rmdup_emit", _int, [_vp, _u64, _u64, _int, C.POINTER(SplitInfo)]),
    ("hpn_bam_rmdup_blocks", _int, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("hpn_bam_rmdup_payload_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_bam_rmdup_stored_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_depth_begin", _int, [_vp, _i32, _u32, _u32]),
    ("hpn_depth_begin_w", _int, [_vp, _i32, _u32, _u32, _u32]),
    ("hpn_depth_progress", _int, [_vp, C.POINTER(_u64)]),
    ("hpn_depth_add", _int, [_vp, C.POINTER(BamBatch)]),
    ("hpn_depth_add_dev", _int, [_vp, C.POINTER(BamBatch)]),
    ("hpn_depth_finish", _int, [_vp, _u32, _vp, _u64, C.POINTER(_u64), _vp]),
    ("hpn_depth_bedgraph_format", _int, [_vp, C.c_char_p, C.POINTER(_u64)]),
    ("hpn_depth_bedgraph_read", _int, [_vp, _u64, _vp, _u64]),
    ("hpn_depth_bedgraph_dev", _int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("hpn_window_begin", _int, [_vp, _i32, _vp, _u32]),
    ("hpn_window_add", _int, [_vp, C.POINTER(BamBatch)]),
    ("hpn_window_add_dev", _int, [_vp, C.POINTER(BamBatch)]),
    ("hpn_window_finish", _int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    ("hpn_comm_unique_id", _int, [_vp]),
    ("hpn_comm_init", _int, [_vp, _int, _int, _vp]),
    ("hpn_comm_destroy", _int, [_vp]),
    ("hpn_allreduce_u64", _int, [_vp, _vp, _sz]),
    ("hpn_comm_init_all", _int, [C.POINTER(_vp), _int]),
    ("hpn_allreduce_u64_all", _int, [C.POINTER(_vp), C.POINTER(_vp), _int, _sz]),
    ("hpn_comm_library", C.c_char_p, []),
    ("hpn_comm_count", _int, [_vp, C.POINTER(_int)]),
    ("hpn_synth_fastq_dev", _int, [_vp, _u64, _u64, _u64, _u32, _vp, _vp, _vp]),
]

_lib = None


def lib():
    """Load libhpngs.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C highperformancengs_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        try:
            fn = getattr(L, name)  # AttributeError if the ABI and the header drift apart
        except AttributeError:
            if os.environ.get("HPN_LIB"):   # an A/B build of an older tree (scripts/ab_build.sh) may lack the newest entry points
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    if L.hpn_abi_version() != 18:
        raise RuntimeError("libhpngs.so ABI version mismatch")
    _lib = L
    return L


def _strerror(status):
    try:
        return lib().hpn_strerror(status).decode()
    except Exception:
        return "?"
