/*
 * hpngs.h -- C ABI of the MI355X (gfx950) scan kernels that stand in for the
 * per-record loops of HighPerformanceNGS' fastq_count / fastq_trim / bam2depth /
 * bam_sliding_count.
 *
 * The reference has no library API; its seams are three C call signatures
 * (SURVEY.md §8b).  Each entry point below names the reference function it
 * replaces (file:line relative to the reference checkout).  Conventions:
 *   - plain C types, no exceptions; every call returns HPN_OK (0) or a negative
 *     hpn_status; hpn_ctx_last_error() has the detail text;
 *   - one hpn_ctx per GPU, used by one host thread at a time;
 *   - "host" entry points take caller-owned host buffers, copy, launch, wait and
 *     ADD into caller-owned accumulators, exactly like count_read adds into the
 *     arrays its caller zeroed (fastq_count_kthread.c:116,126);
 *   - "_dev" entry points take device pointers (hipMalloc / hpn_dev_malloc /
 *     torch tensors), enqueue on the context's stream and return immediately;
 *     results are collected by the matching "_fetch" call;
 *   - there is NO CPU fallback: without a usable GPU every compute call fails
 *     with HPN_E_NODEVICE.
 */
#ifndef HPNGS_H
#define HPNGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPN_ABI_VERSION 18
#define HPN_LEN_BINS 512   /* SeqLen[512]       fastq_count.c:111 */
#define HPN_QUAL_ROWS 128  /* Quality[128][512] fastq_count.c:110 */
#define HPN_NUC_CODES 5    /* T,C,A,G,N         Rgzfastq_uniq.c:97-108 */

typedef enum hpn_status {
    HPN_OK = 0,
    HPN_E_NODEVICE = -1, /* no HIP device / runtime */
    HPN_E_HIP = -2,      /* a HIP call failed */
    HPN_E_ARG = -3,      /* bad argument */
    HPN_E_DOMAIN = -4,   /* input on which the reference has undefined behaviour
                            (read length >= 512, quality byte >= 128, position >= 2^28 ...) */
    HPN_E_NOMEM = -5,
    HPN_E_STATE = -6,    /* call sequence error (e.g. depth_add before depth_begin) */
    HPN_E_RCCL = -7,
    HPN_E_CAPACITY = -8, /* caller-provided output buffer too small; required size reported */
    HPN_E_PARTIAL = -9   /* a grouped collective failed after some ranks were enqueued: the vectors
                            may or may not hold sums and must not be added again (abandon the input) */
} hpn_status;

typedef struct hpn_ctx hpn_ctx;

/* ---- library / context ----------------------------------------------------- */
int hpn_abi_version(void);
const char *hpn_strerror(int status);
int hpn_device_count(int *n);
/* `device` = HIP ordinal.  Creates the context's own non-blocking stream. */
int hpn_ctx_create(int device, hpn_ctx **ctx);
int hpn_ctx_destroy(hpn_ctx *ctx);
/* Run on a caller-owned hipStream_t instead (e.g. torch's current stream);
 * NULL restores the context's own stream. */
int hpn_ctx_set_stream(hpn_ctx *ctx, void *hip_stream);
int hpn_ctx_sync(hpn_ctx *ctx);
/* The HIP ordinal the context was created on (a helper context for uploads beside it: host/gz_gpu.hpp). */
int hpn_ctx_device(const hpn_ctx *ctx, int *device);
/* The device's PCI address ("0000:c1:00.0" + NUL; HPN_E_ARG when `len` < 16).  What a host needs to keep the threads that
 * feed the device on the CPUs next to it: /sys/bus/pci/devices/<address>/local_cpulist (host/cpus.hpp: on a two-socket box a
 * reader on the far socket moves 38 GB/s to the device, one on the near socket 51 -- profiles/r05/numa_probe.txt).  The
 * reference has no counterpart: its readers are the threads of kt_for, wherever the scheduler puts them (klib/kthread.c:48). */
int hpn_ctx_pci_address(const hpn_ctx *ctx, char *buf, int len);
const char *hpn_ctx_last_error(const hpn_ctx *ctx);
/* Milliseconds the device spent in the most recent kernel launch group of the
 * given family, measured with hipEvents on the context's stream (valid after
 * the matching fetch/sync). Families: 0 tally, 1 trim, 2 depth, 3 window,
 * 4 text framing, 5 BGZF inflate, 6 record index of hpn_bam_raw_index_dev (its four
 * kernels and the host's look at the counts between them), 7 the field view
 * hpn_window_add_raw_dev makes of the indexed records. */
int hpn_ctx_last_kernel_ms(hpn_ctx *ctx, int family, float *ms);

/* ---- memory helpers (thin wrappers; callers may use their own allocator) ---- */
int hpn_dev_malloc(hpn_ctx *ctx, size_t bytes, void **dptr);
int hpn_dev_free(hpn_ctx *ctx, void *dptr);
int hpn_host_malloc(hpn_ctx *ctx, size_t bytes, void **hptr); /* pinned */
int hpn_host_free(hpn_ctx *ctx, void *hptr);
int hpn_memcpy_h2d(hpn_ctx *ctx, void *dst, const void *src, size_t bytes); /* async on ctx stream */
int hpn_memcpy_d2h(hpn_ctx *ctx, void *dst, const void *src, size_t bytes); /* async on ctx stream */
int hpn_memcpy_d2d(hpn_ctx *ctx, void *dst, const void *src, size_t bytes); /* async on ctx stream; same device */
int hpn_dev_mem_info(hpn_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes); /* of the context's device, now */

/* ---- fastq_count: replaces count_read's scan loop ------------------------------
 * fastq_count.c:112-119 / fastq_count_kthread.c:126-135 (+ AssignQuality :29-35).
 *
 * A batch is structure-of-arrays: record i owns bytes [off[i], off[i+1]) of
 * `qual` (the first seqLen bytes of its quality line) and, optionally, of
 * `base` (its sequence line).  Adds into `acc`:
 *   seqlen[l]            += #records of length l            (SeqLen[512])
 *   total, q20, q30      += #bytes, #bytes >= 53, >= 63     (statQ(...,53,...,63,...), :37-47,124)
 *   qual_hist[q*512+pos] += 1 per byte        if non-NULL   (Quality[128][512])
 *   nuc_hist[c*512+pos]  += 1 per base        if non-NULL and `base` given
 *                           (c: T0 C1 A2 G3 N4, any other byte counts as T,
 *                            Rgzfastq_uniq.c:97-108)
 * Domain (else HPN_E_DOMAIN, accumulators untouched): every length < 512,
 * every quality byte < 128. */
typedef struct hpn_tally {
    uint64_t seqlen[HPN_LEN_BINS];
    uint64_t total, q20, q30;
    uint64_t *qual_hist; /* [HPN_QUAL_ROWS * HPN_LEN_BINS] or NULL */
    uint64_t *nuc_hist;  /* [HPN_NUC_CODES * HPN_LEN_BINS] or NULL */
} hpn_tally;

#define HPN_TALLY_QUAL_HIST 1u /* also build Quality[128][512] */
#define HPN_TALLY_NUC_HIST 2u  /* also build Nucleotide[5][512] (needs base) */

int hpn_fastq_tally(hpn_ctx *ctx, const uint8_t *qual, const uint8_t *base_or_null,
                    const uint64_t *off, uint64_t n_records, hpn_tally *acc);
/* Device-resident batch; accumulates into the context's device accumulators. */
int hpn_fastq_tally_dev(hpn_ctx *ctx, const uint8_t *d_qual, const uint8_t *d_base_or_null,
                        const uint64_t *d_off, uint64_t n_records, uint32_t flags);
/* Wait, add the device accumulators into `acc`, zero them. */
int hpn_fastq_tally_fetch(hpn_ctx *ctx, hpn_tally *acc);
/* The raw device accumulator block (uint64_t[HPN_TALLY_WORDS], layout below) for
 * callers that reduce it across GPUs themselves (RCCL all-reduce). */
#define HPN_TALLY_W_SEQLEN 0                                    /* [512] */
#define HPN_TALLY_W_TOTAL 512
#define HPN_TALLY_W_Q20 513
#define HPN_TALLY_W_Q30 514
#define HPN_TALLY_W_BAD 515                                     /* domain violations seen */
#define HPN_TALLY_W_QUAL 516                                    /* [128*512] */
#define HPN_TALLY_W_NUC (516 + HPN_QUAL_ROWS * HPN_LEN_BINS)    /* [5*512] */
#define HPN_TALLY_WORDS (HPN_TALLY_W_NUC + HPN_NUC_CODES * HPN_LEN_BINS)
int hpn_fastq_tally_devptr(hpn_ctx *ctx, uint64_t **d_acc);

/* ---- Rfastqc tally: the per-read statistics of the R plugin -------------
 * Rgzfastq_uniq.c: STATSEQ (:50-57), AssignQuality (:42-48), Length (:174), as returned by
 * qsort_hash_count (:250) in list elements 2..5 -- in the plugin's own layouts:
 *   quality[q + 128*pos]      += 1 per quality byte q at cycle pos          int[128*300]
 *   nucleotide[5*pos + code]  += 1 per base (T/U 0, C 1, A 2, G 3, N '.' 4,   int[5*300]
 *                                 every other byte 0; :97-108)
 *   length[len - 1]           += 1 per read                                 int[300]
 *   gc[i]                      = #{'G','C'} / len of read i, as double       double[n]
 * Adds into quality / nucleotide / length (the plugin callocs them, :37-40) and writes
 * gc.  Any of the four pointers may be NULL.  The duplicate-count vector (list element
 * 1) and a path from a file are hpn_rfastqc_* below; this entry point takes arrays the caller
 * has framed.
 * Domain (else HPN_E_DOMAIN): 1 <= len <= 300 (MaxLen; the plugin writes out of bounds
 * otherwise), quality byte < 128. */
#define HPN_RQC_MAXLEN 300
typedef struct hpn_rqc {
    int32_t *quality;
    int32_t *nucleotide;
    int32_t *length;
    double *gc;
} hpn_rqc;
int hpn_fastq_rqc(hpn_ctx *ctx, const uint8_t *seq, const uint8_t *qual, const uint64_t *off,
                  uint64_t n_records, hpn_rqc *out);
/* The GC-fraction part alone, on device-resident arrays (async on the context's stream). */
int hpn_fastq_read_gc_dev(hpn_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_records,
                          double *d_gc);

/* ---- fastq_trim: replaces readNextNode's cut --------------------------------------
 * fastq_trim.c:76-77,83-84: out = line[min(S,len) .. min(E,len)) for the sequence
 * and the quality line of every record.  out_off[0] = 0, out_off[i+1] = running
 * total; out_seq/out_qual are packed.  Capacity of out_seq/out_qual: off[n]-off[0]
 * bytes is always enough.  Domain: 0 <= S <= E. */
int hpn_fastq_trim(hpn_ctx *ctx, const uint8_t *seq, const uint8_t *qual, const uint64_t *off,
                   uint64_t n_records, int32_t S, int32_t E, uint8_t *out_seq, uint8_t *out_qual,
                   uint64_t *out_off);
int hpn_fastq_trim_dev(hpn_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual,
                       const uint64_t *d_off, uint64_t n_records, int32_t S, int32_t E,
                       uint8_t *d_out_seq, uint8_t *d_out_qual, uint64_t *d_out_off);

/* ---- EXTENSION: quality-threshold trim points ----------------------------------------
 * No reference counterpart: the reference's fastq_trim is the fixed-cycle cut above
 * (SURVEY.md §0.1 D3); BASELINE.json's north_star asks for a quality-threshold
 * trim-point scan as well.  Definition used here, per record:
 *   beg = index of the first quality byte >= threshold
 *   end = 1 + index of the last quality byte >= threshold     (beg = end = 0 if none)
 * hpn_fastq_trim_points cuts every record to its own [beg[i], end[i]) (clamped to the
 * record), with the same packed outputs as hpn_fastq_trim. */
int hpn_fastq_qtrim_points(hpn_ctx *ctx, const uint8_t *qual, const uint64_t *off, uint64_t n_records,
                           uint32_t threshold, uint32_t *beg, uint32_t *end);
int hpn_fastq_qtrim_points_dev(hpn_ctx *ctx, const uint8_t *d_qual, const uint64_t *d_off, uint64_t n_records,
                               uint32_t threshold, uint32_t *d_beg, uint32_t *d_end);
int hpn_fastq_trim_points(hpn_ctx *ctx, const uint8_t *seq, const uint8_t *qual, const uint64_t *off,
                          uint64_t n_records, const uint32_t *beg, const uint32_t *end, uint8_t *out_seq,
                          uint8_t *out_qual, uint64_t *out_off);
int hpn_fastq_trim_points_dev(hpn_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, const uint64_t *d_off,
                              uint64_t n_records, const uint32_t *d_beg, const uint32_t *d_end,
                              uint8_t *d_out_seq, uint8_t *d_out_qual, uint64_t *d_out_off);

/* ---- raw FASTQ text front end: the 4 x gzgets framing on the device ----------------------
 * fastq_count.c:112-118 and fastq_trim.c:67-89 frame a stream with four gzgets()
 * calls per record into one 1024-byte buffer.  On REGULAR text that loop is a pure
 * function of the newline positions, and these calls evaluate it on the GPU from the
 * raw (decompressed) bytes: no host pass over the text at all.  Regular means
 *   - no NUL byte, every line at most 1022 characters + '\n' (gzgets would split it);
 *   - the stream ends with a whole record (count: the very last '\n' may be missing,
 *     the reference then drops nothing it would tally);
 *   - count: the quality line is not shorter than the sequence line (the reference
 *     would tally stale buffer bytes), read length < 512;
 *   - trim: sequence and quality line have the same length, S <= every read's length.
 * Anything else is DETECTED, never mis-framed: the call reports the reasons in
 * info->irregular, adds nothing, and closes the text stream; the caller then frames
 * that input with the exact gzgets emulation (csrc/host/fastq_reader.hpp) and
 * hpn_fastq_tally / hpn_fastq_trim.
 *
 * A stream is fed in chunks of any size (< 2^31 bytes) cut anywhere; the bytes of an
 * unfinished trailing record stay on the device and are prepended to the next chunk.
 * `text` may be a host pointer (pinned: the copy is asynchronous; the call returns
 * after the copy has completed, so the buffer may be reused at once) or a device
 * pointer.  `last` != 0 marks the final chunk (nbytes may be 0). */
typedef struct hpn_text_info {
    uint64_t n_records;   /* records framed by this call */
    uint64_t n_bytes;     /* count: sum of their lengths; trim: bytes of output text */
    uint64_t carry_bytes; /* tail bytes kept for the next chunk */
    uint32_t irregular;   /* HPN_TEXT_* reasons, 0 = chunk processed */
    uint32_t reserved;
} hpn_text_info;

#define HPN_TEXT_NUL 1u        /* NUL byte in the text */
#define HPN_TEXT_LONG_LINE 2u  /* line of 1023+ characters */
#define HPN_TEXT_RAGGED 4u     /* quality line shorter than (trim: different from) the sequence line */
#define HPN_TEXT_PARTIAL 8u    /* stream ends inside a record */
#define HPN_TEXT_LEN 16u       /* read of 512+ bases (count) */
#define HPN_TEXT_DENSE 32u     /* more than one line per 4 bytes: not worth indexing */
#define HPN_TEXT_STALE 64u     /* trim: S beyond a read's end (the reference copies what the record's
                                  earlier lines left in its buffer; the host framer reproduces that) */
#define HPN_TEXT_SHORT_QUAL 128u /* uniq: quality line two or more bytes shorter than the sequence (the reference sums
                                  bytes outside its buffer) */
#define HPN_TEXT_KSEQ 256u     /* kseq: the text has neither of the two shapes the device frames (hpn_kseq_*) */
/* The writable bytes hpn_fastq_text_count_inplace needs in front of the text it frames where it lies. */
#define HPN_TEXT_INPLACE_PAD 8192u

int hpn_fastq_text_begin(hpn_ctx *ctx);
/* count_read's loop: adds into the context's device accumulators exactly like
 * hpn_fastq_tally_dev (collect with hpn_fastq_tally_fetch).  tally_flags: HPN_TALLY_*. */
int hpn_fastq_text_count(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, uint32_t tally_flags,
                         hpn_text_info *info);
/* The same for text that lies on the device already (a batch inflated there: hpn_gz_inflate_dev, hpn_bgzf_inflate_dev),
 * framed WHERE IT LIES: d_text must have HPN_TEXT_INPLACE_PAD writable bytes of device memory in front of it (the carried bytes of the
 * chunk before are laid there) and 64 readable bytes behind d_text + nbytes; nothing else is copied.  The text may be
 * overwritten as soon as the call returns.  Chunks framed in place and chunks framed by hpn_fastq_text_count may follow each
 * other in one stream. */
int hpn_fastq_text_count_inplace(hpn_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int last, uint32_t tally_flags,
                                 hpn_text_info *info);
/* gzfastq_sample.c:214-225 count_read: the same four gzgets per record with nothing but i++ in the
 * loop (its "total_reads_num").  Frames the chunk like hpn_fastq_text_count and tallies nothing:
 * info->n_records of every chunk add up to the reference's i (= the ReadCount column of fastq_count
 * for the same file).  Irregular text is reported the same way; the host framer then counts. */
int hpn_fastq_text_records(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, hpn_text_info *info);
/* readNextNode + fprintf("%s\n%s\n+\n%s\n") (fastq_trim.c:67-89,101): writes the
 * trimmed records of this chunk as text into out_text (host or device pointer,
 * capacity out_cap; nbytes + 8192 always suffices). */
int hpn_fastq_text_trim(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, int32_t S, int32_t E,
                        void *out_text, uint64_t out_cap, hpn_text_info *info);

/* gzfastq_sample.c: a subsample of the stream's records as text.  Records are framed as readNextNode frames them
 * (:315-335, the four gzgets of fastq_trim.c); record i (1-based over the whole stream, counted across the chunks since
 * hpn_fastq_text_begin) is kept by one of two rules and written as printNode writes it (:30-37): "name_i\nseq\n+\n" + the
 * quality line as read (a last line without '\n' stays without), or with `fasta` ">name_i\nseq\n" (the name keeps its '@').
 *   HPN_SAMPLE_FRACTION  filter_reads (:150-153): keep iff ((X31(name) + seed_add) & 0xffffff) < threshold, X31 the string hash
 *                        of khash.h:336-341 over the whole name line without its '\n' (bytes as signed chars).  The
 *                        reference's test (k & 0xffffff) / 2^24 < frac is this one with threshold = ceil(frac * 2^24).
 *   HPN_SAMPLE_PICKS     get_number_from_file (:253-264): keep iff the record's 0-based ordinal is in `picks`, a sorted list
 *                        of ordinals over the whole stream in HOST memory (n_picks of them; the list must stay the same
 *                        for all chunks of a stream). */
#define HPN_SAMPLE_FRACTION 1u
#define HPN_SAMPLE_PICKS 2u
typedef struct hpn_sample_rule {
    uint32_t mode;          /* HPN_SAMPLE_FRACTION or HPN_SAMPLE_PICKS */
    uint32_t fasta;         /* 0: FASTQ records, 1: FASTA records */
    uint32_t seed_add;      /* fraction rule */
    uint32_t threshold;     /* fraction rule: 0 .. 2^24 (2^24 keeps every record) */
    const uint64_t *picks;  /* pick rule */
    uint64_t n_picks;
    uint64_t first_ordinal; /* 0-based ordinal of the STREAM's first record: 0, or where the stream this one continues ended */
} hpn_sample_rule;
typedef struct hpn_sample_info {
    uint64_t n_records;   /* records framed in this chunk */
    uint64_t n_kept;      /* ... of which kept */
    uint64_t n_bytes;     /* bytes written to out_text */
    uint64_t carry_bytes; /* tail bytes kept for the next chunk */
    uint32_t irregular;   /* HPN_TEXT_* reasons, 0 = chunk processed */
    uint32_t reserved;
} hpn_sample_info;
/* Same chunk contract as hpn_fastq_text_trim (chunks cut anywhere, the unfinished record is carried on the device, `text` and
 * `out_text` host or device pointers, `last` closes the stream).  Irregular text -- NUL byte, line of 1023+ characters, stream
 * ending inside a record, HPN_TEXT_DENSE -- is reported in info->irregular and nothing of the chunk is written; a quality line
 * of another length than the sequence line is regular here (HPN_TEXT_RAGGED / HPN_TEXT_STALE are never raised: whole lines are
 * copied).  kept_ordinals (host or device pointer, or NULL): receives the 0-based ordinals of the kept records in order --
 * the pick list for the mate file (-2), whose records are written exactly when the first file's are.
 * Capacities: a kept record outgrows its input by at most 21 bytes ('_' and up to 20 digits), one more where the input's third
 * line is empty, one more for FASTA's '>': out_cap = nbytes + 8192 + 23 * (records in the chunk) always suffices, and so does
 * kept_cap = (nbytes + 8192) / 4.  What does not fit is HPN_E_CAPACITY: nothing is written and the stream is closed. */
int hpn_fastq_text_sample(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, const hpn_sample_rule *rule,
                          void *out_text, uint64_t out_cap, uint64_t *kept_ordinals, uint64_t kept_cap, hpn_sample_info *info);

/* ---- gzfastq_uniq.c: one record per distinct sequence ------------------------------------------------
 * The reads of one stream (or the pairs of two) are collapsed by their sequence (pairs: by both sequences joined, so
 * "AC" + "G" and "A" + "CG" are one key).  Per key: the number of records, and as representative the EARLIEST record
 * whose quality sum (the first seq_len bytes of the quality string, both mates added) is the greatest.  Records are
 * framed as readNextNode frames them (gzfastq_uniq.c:170-192): name, sequence and quality are their lines without the
 * last byte -- a '\r' stays, a last line without '\n' loses a real character; a lone line without '\n' behind the
 * last record is no record.  An output record is "name\tcount\nsequence\n+\nquality\n".
 *
 *   hpn_fastq_uniq_begin   opens a session (closing the context's earlier one).  `paired`: two streams, mate 0 and 1.
 *                          max_bytes: the most text (both mates, as fed) the device store may hold; 0 = half of the
 *                          device memory that is free now, the other half being the reserve for the store's growth and
 *                          the sorts' arrays.  hash_bits: 0 = records are grouped by all 64 bits of the grouping hash;
 *                          1 .. 63 keeps only that many -- a verification aid: the outputs must not depend on it,
 *                          because keys are always compared by their bytes.
 *   hpn_fastq_uniq_add     one chunk of mate `mate` (the chunk contract of hpn_fastq_text_sample: cut anywhere, host or
 *                          device pointer, `last` closes the mate's stream; the mates may be fed in any interleaving).
 *                          Irregular text -- HPN_TEXT_NUL, _LONG_LINE, _PARTIAL, _DENSE, _SHORT_QUAL -- is reported in
 *                          info->irregular and closes the session.  A chunk with which the store would outgrow max_bytes:
 *                          HPN_E_CAPACITY (the message tells how much was needed), session closed.  2^31 or more
 *                          records: HPN_E_DOMAIN.
 *   hpn_fastq_uniq_finish  after every mate's last chunk: groups, orders, fills *result.  Pairs: reading stops at the
 *                          first ordinal whose mate is missing (mate 0 has more records) or whose names differ within
 *                          the bytes in front of name 0's first space (no space: the names must be equal);
 *                          result->unmatched is that ordinal (-1: none), unmatched_name the name of mate 0 there, and
 *                          n_records counts the pairs in front of it.
 *   hpn_fastq_uniq_write   copies up to `cap` bytes of an output, from byte `offset` on, to `out` (host or device).
 *                          HPN_UNIQ_TABLE_ORDER: the order in which the reference walks its hash table (mate 0, and
 *                          mate 1 of a paired session; result->out_bytes[mate] bytes).  HPN_UNIQ_KEY_ORDER: single-end
 *                          only, keys ascending by memcmp, then length (out_bytes[0] bytes as well).  Reading one
 *                          output front to back before the next one costs one formatting pass per output. */
typedef struct hpn_uniq_info {
    uint64_t n_records;   /* records framed by this call */
    uint64_t store_bytes; /* text held by the store (both mates) after this call */
    uint32_t irregular;   /* HPN_TEXT_* reasons, 0 = chunk processed */
    uint32_t reserved;
} hpn_uniq_info;
typedef struct hpn_uniq_result {
    uint64_t n_records;    /* records (pairs) that were keyed */
    uint64_t n_unique;     /* distinct keys */
    uint64_t hash_size;    /* the size the reference's table would have ("hash size: ") */
    int64_t unmatched;     /* pairs: the first ordinal without a matching mate, else -1 */
    uint64_t out_bytes[2]; /* bytes of the outputs of mate 0 and mate 1 */
    uint64_t hash_clashes; /* records whose grouping hash equalled their neighbour's over different bytes */
    char unmatched_name[1024];
} hpn_uniq_result;
#define HPN_UNIQ_TABLE_ORDER 0
#define HPN_UNIQ_KEY_ORDER 1
int hpn_fastq_uniq_begin(hpn_ctx *ctx, int paired, uint64_t max_bytes, uint32_t hash_bits);
int hpn_fastq_uniq_add(hpn_ctx *ctx, int mate, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info);
int hpn_fastq_uniq_finish(hpn_ctx *ctx, hpn_uniq_result *result);
int hpn_fastq_uniq_write(hpn_ctx *ctx, int which_output, int mate, uint64_t offset, void *out, uint64_t cap,
                         uint64_t *written);
/* The stable radix sort behind it on its own: n < 2^31 pairs, ascending by key, equal keys in their given order.
 * keys and vals: host or device pointers, sorted in place. */
int hpn_sort_pairs_u64(hpn_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t n);
/* hpn_sort_pairs_u64 by the key bits [begin_bit, end_bit) only (0 <= begin_bit <= end_bit <= 64); pairs equal in those bits
 * keep their given order.  The keys come back whole, not masked. */
int hpn_sort_pairs_u64_bits(hpn_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t n, int begin_bit, int end_bit);
/* ... by the bytes of the key whose bit is set in digits (bit d: key bits [8d, 8d+8)), digits < 256. */
int hpn_sort_pairs_u64_digits(hpn_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t n, uint32_t digits);
/* The prefix scan behind the families on its own: out[i] = in[0] + ... + in[i-1] for i in 0..n (n + 1 entries; n = 0 writes
 * out[0] = 0 and takes in == NULL).  (in_bits, out_bits) is one of (32,32), (32,64), (64,64); a 32-bit out holds the sum
 * modulo 2^32, and the total of a 64-bit one must stay below 2^62.  Host or device pointers; in and out must not overlap.
 * n < 2^31.  All four: HPN_E_ARG for what is outside the above, HPN_E_DOMAIN at n >= 2^31, HPN_E_STATE while a
 * hpn_fastq_uniq session is collecting text (they run in its work space). */
int hpn_excl_scan(hpn_ctx *ctx, const void *in, int in_bits, void *out, int out_bits, uint64_t n);

/* ---- gzfastq_uniqQ.c: one group per distinct sequence, every copy's quality line kept ---------------------
 * The reads of one stream are collapsed by their sequence like hpn_fastq_uniq_* collapses them, framed by the same
 * readNextNode (gzfastq_uniqQ.c:181-203), but every record stays in its key's list, new records at the head
 * (list_add_data, list.c; gzfastq_uniqQ.c:220, :229).  An output group is "name\tcount\nsequence\n+\n" with the name of the
 * LAST record read that carries the sequence (:86), and then one "quality\n" per member, from the last record read to the
 * first (:67-76).  The quality sum (:217) is never printed: a quality line shorter than its sequence is regular here.
 *
 *   hpn_fastq_uniqq_begin   opens a session (closing the context's earlier one; a hpn_fastq_uniq session is another one and
 *                           stays).  max_bytes and hash_bits: as for hpn_fastq_uniq_begin.
 *   hpn_fastq_uniqq_add     one chunk (the chunk contract of hpn_fastq_uniq_add: cut anywhere, host or device pointer, `last`
 *                           closes the stream).  Irregular text -- HPN_TEXT_NUL, _LONG_LINE, _PARTIAL, _DENSE -- is reported in
 *                           info->irregular and closes the session; HPN_TEXT_SHORT_QUAL is never raised.  HPN_E_CAPACITY and
 *                           HPN_E_DOMAIN (2^31 or more records) as there.
 *   hpn_fastq_uniqq_finish  after the last chunk: groups, orders, fills *result.  hash_size: the reference only ever calls
 *                           dictAdd (:221), so its table has the smallest power of two >= max(n_unique, 4) slots (0 without a
 *                           record).
 *   hpn_fastq_uniqq_write   copies up to `cap` bytes of an output (result->out_bytes in either order), from byte `offset` on, to
 *                           `out` (host or device).  HPN_UNIQQ_KEY_ORDER: keys ascending by memcmp, then length (-S,
 *                           compare_hashed_key :246-248).  HPN_UNIQQ_COUNT_ORDER: count descending, equal counts in the order in
 *                           which the reference walks its table (-C, compare_hashed_data_count :242-244 under glibc's stable
 *                           qsort over dump_dict's array :250-261).  Reading one output front to back before the other costs
 *                           one formatting pass per output. */
typedef struct hpn_uniqq_result {
    uint64_t n_records;    /* records that were keyed */
    uint64_t n_unique;     /* distinct keys */
    uint64_t hash_size;    /* the size the reference's table would have ("hash size: ") */
    uint64_t hash_clashes; /* records whose grouping hash equalled their neighbour's over different bytes */
    uint64_t out_bytes;    /* bytes of the output (the same in both orders) */
    uint32_t max_count;    /* the largest group */
    uint32_t reserved;
} hpn_uniqq_result;
#define HPN_UNIQQ_KEY_ORDER 0
#define HPN_UNIQQ_COUNT_ORDER 1
int hpn_fastq_uniqq_begin(hpn_ctx *ctx, uint64_t max_bytes, uint32_t hash_bits);
int hpn_fastq_uniqq_add(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info);
int hpn_fastq_uniqq_finish(hpn_ctx *ctx, hpn_uniqq_result *result);
int hpn_fastq_uniqq_write(hpn_ctx *ctx, int which_output, uint64_t offset, void *out, uint64_t cap, uint64_t *written);

/* ---- gzfastq_uniq_sort.c: one record per distinct sequence, most frequent first ---------------------------
 * The reads of one stream (or the pairs of two) are collapsed by their sequence (pairs: by both sequences joined) like
 * hpn_fastq_uniq_* collapses them, framed by the same readNextNode (gzfastq_uniq_sort.c:67-88); a quality line shorter than its
 * sequence is regular (nothing reads it against the sequence).  Per key: the number of records, and as representative the
 * FIRST record that carries it (:147-159).  The keys come by count descending; equal counts in the order in which the
 * reference walks its table (hashtbl.c): a table of S = (size_t)(1.34 * e) slots that never resizes, e = the groups of four
 * lines that count_read (:174-185) sees in mate 0 -- one open line behind the last record counts --, slot =
 * djb2 over 64 bits modulo S, every chain newest key first.  An output record is "name\tcount\nSEQ\n+\nquality\n"; SEQ of
 * mate 0 is the first seq_len bytes of the joined key (a shorter key whole), SEQ of mate 1 the bytes behind them; seq_len is the
 * length of the first mate-0 sequence that is not empty (:129).
 *
 *   hpn_fastq_usort_begin   opens a session (closing the context's earlier one; sessions of hpn_fastq_uniq_* and _uniqq_* are
 *                           others and stay).  paired, max_bytes and hash_bits: as for hpn_fastq_uniq_begin.
 *   hpn_fastq_usort_add     the chunk contract of hpn_fastq_uniq_add.  Irregular text -- HPN_TEXT_NUL, _LONG_LINE, _PARTIAL,
 *                           _DENSE -- is reported in info->irregular and closes the session; HPN_TEXT_SHORT_QUAL is never raised.
 *                           HPN_E_CAPACITY and HPN_E_DOMAIN (2^31 or more records) as there.
 *   hpn_fastq_usort_finish  after every mate's last chunk: groups, orders, fills *result.  Pairs stop at the first ordinal
 *                           without a matching mate as in hpn_fastq_uniq_finish.  Where the reference has no answer the call
 *                           returns HPN_E_DOMAIN, result->no_answer tells why and the session is closed:
 *                           HPN_USORT_FEW_READS  e < 10 and at least one record: the reference divides by e / 10 (:161);
 *                           HPN_USORT_LONG_KEY   a pair's joined sequences have more than 1023 bytes (pair_seq, :125);
 *                           HPN_USORT_SHORT_KEY  a pair's joined sequences have fewer than seq_len bytes (key + strLen, :227).
 *   hpn_fastq_usort_write   copies up to `cap` bytes of the output of mate `mate` (result->out_bytes[mate]), from byte `offset`
 *                           on, to `out` (host or device).  Reading one output front to back before the other costs one
 *                           formatting pass per output. */
typedef struct hpn_usort_result {
    uint64_t n_records;    /* records (pairs) that were keyed ("total reads = ") */
    uint64_t n_unique;     /* distinct keys */
    uint64_t table_reads;  /* e ("total_reads_num: ") */
    uint64_t hash_size;    /* S ("hash size: ") */
    int64_t unmatched;     /* pairs: the first ordinal without a matching mate, else -1 */
    uint64_t out_bytes[2]; /* bytes of the outputs of mate 0 and mate 1 */
    uint64_t hash_clashes; /* records whose grouping hash equalled their neighbour's over different bytes */
    uint32_t max_count;    /* the largest group */
    uint32_t seq_len;      /* strLen */
    uint32_t no_answer;    /* 0, or HPN_USORT_* with HPN_E_DOMAIN */
    uint32_t reserved;
    char unmatched_name[1024];
} hpn_usort_result;
#define HPN_USORT_FEW_READS 1u
#define HPN_USORT_LONG_KEY 2u
#define HPN_USORT_SHORT_KEY 3u
int hpn_fastq_usort_begin(hpn_ctx *ctx, int paired, uint64_t max_bytes, uint32_t hash_bits);
int hpn_fastq_usort_add(hpn_ctx *ctx, int mate, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info);
int hpn_fastq_usort_finish(hpn_ctx *ctx, hpn_usort_result *result);
int hpn_fastq_usort_write(hpn_ctx *ctx, int mate, uint64_t offset, void *out, uint64_t cap, uint64_t *written);

/* ---- gzfastq_sort.c: the whole file ordered by name or by sequence ---------------------------------------
 * The records of one stream, framed as readNextNode frames them (see above), in ascending order of their KEY LINE -- the
 * whole name line with its '@' and comment (by_name) or the sequence line: first by its length, then by its bytes compared as
 * unsigned; records with equal keys stay in input order (the reference's qsort is glibc's merge sort).  An output record is
 * "name\nsequence\n+\nquality\n".
 *
 *   hpn_fastq_sort_begin   opens a session (closing the context's earlier one).  max_bytes: as for hpn_fastq_uniq_begin.
 *   hpn_fastq_sort_add     one chunk (the chunk contract of hpn_fastq_uniq_add: cut anywhere, host or device pointer, `last`
 *                          closes the stream).  Irregular text -- HPN_TEXT_NUL, _LONG_LINE, _PARTIAL, _DENSE -- is reported in
 *                          info->irregular and closes the session; a quality line shorter than its sequence is regular here
 *                          (nothing reads it against the sequence).  HPN_E_CAPACITY and HPN_E_DOMAIN (2^31 or more records)
 *                          as there.
 *   hpn_fastq_sort_finish  after the last chunk: orders the records, formats the output on the device, fills *result.
 *                          The order is built most significant bytes first: round 0 sorts all records by length and their
 *                          first 6 bytes, round k >= 1 only the records of runs that are still undecided, by their next 8
 *                          bytes.  result->rounds counts the rounds (round 0 included; 0 without records),
 *                          result->refined the records that rounds 1, 2, ... worked on, added up.
 *   hpn_fastq_sort_write   copies up to `cap` bytes of the output (result->out_bytes in all), from byte `offset` on, to `out`
 *                          (host or device). */
typedef struct hpn_sort_info {
    uint64_t n_records;   /* records framed by this call */
    uint64_t store_bytes; /* text held by the store after this call */
    uint32_t irregular;   /* HPN_TEXT_* reasons, 0 = chunk processed */
    uint32_t reserved;
} hpn_sort_info;
typedef struct hpn_sort_result {
    uint64_t n_records; /* records ordered */
    uint64_t out_bytes; /* bytes of the output */
    uint64_t refined;   /* sum over the rounds k >= 1 of the records they sorted */
    uint32_t rounds;    /* rounds run, round 0 included */
    uint32_t lone_line; /* 1: a line without '\n' stands behind the last record -- no record (gzeof is true after its gzgets),
                           but the reference's count_read counts it */
} hpn_sort_result;
int hpn_fastq_sort_begin(hpn_ctx *ctx, int by_name, uint64_t max_bytes);
int hpn_fastq_sort_add(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, hpn_sort_info *info);
int hpn_fastq_sort_finish(hpn_ctx *ctx, hpn_sort_result *result);
int hpn_fastq_sort_write(hpn_ctx *ctx, uint64_t offset, void *out, uint64_t cap, uint64_t *written);

/* ---- fastq2twobit.c / twoBit2seq.c: the sequences packed to 2 bits per base, and back -----------------------
 * fastq2twobit frames a stream as readNextNode frames it (see above), pushes every record on the front of a list and dumps
 * the list from its head: its output holds the records in REVERSE input order.  A 2-byte header -- (uint8_t)strlen and
 * (uint8_t)packed length of the input's LAST record -- is followed, per record, by (len + 3) >> 2 bytes: four bases per byte,
 * the first in the top bits; 'C'/'c' 1, 'A'/'a' 2, 'G'/'g' 3, every other byte ('T', 'U', 'N', '\r', ...) 0; the tail of a
 * record's last byte is 0; an empty sequence contributes nothing; no record, no byte.  A sequence byte of 0x80 or more indexes
 * the reference's table with a negative number: there is no answer.
 *
 *   hpn_twobit_pack_begin   opens a session (closing the context's earlier one).  max_bytes: as for hpn_fastq_uniq_begin.
 *   hpn_twobit_pack_add     one chunk, the chunk contract of hpn_fastq_sort_add (the same framing, the same info): irregular
 *                           text -- HPN_TEXT_NUL, _LONG_LINE, _PARTIAL, _DENSE -- is reported in info->irregular and closes the
 *                           session.  HPN_E_CAPACITY and HPN_E_DOMAIN (2^31 or more records) as there.
 *   hpn_twobit_pack_finish  after the last chunk: packs on the device, fills *result.  A sequence byte >= 0x80: HPN_E_DOMAIN,
 *                           result->bad_record is the smallest 0-based ordinal of such a record and the session is closed.
 *   hpn_twobit_pack_write   copies up to `cap` bytes of the output (result->out_bytes in all), from byte `offset` on, to `out`
 *                           (host or device).
 *
 * twoBit2seq reads the header and then records of packedLen bytes into a zeroed buffer; of each it prints seqlen characters
 * (0 'T', 1 'C', 2 'A', 3 'G') and '\n'.  Record bytes behind packedLen read as 0: with packedLen < (seqlen + 3) >> 2 the missing
 * bases are 'T', a larger packedLen skips the surplus.
 *
 *   hpn_twobit_unpack       stateless: n_records records of packed_len bytes at `packed` become n_records * (seq_len + 1) bytes
 *                           at `out` (host or device pointers, each on its own); *out_bytes tells how many.  seq_len and
 *                           packed_len are at most 255 (the header's bytes), else HPN_E_ARG.  packed_len == 0 with
 *                           n_records > 0 is HPN_E_ARG (the reference never ends there).  An out_cap below the size needed is
 *                           HPN_E_CAPACITY: *out_bytes holds that size and nothing is written. */
typedef struct hpn_twobit_result {
    uint64_t n_records;  /* records packed */
    uint64_t out_bytes;  /* bytes of the output: 0 without records, else 2 + the packed bytes */
    int64_t bad_record;  /* -1, or with HPN_E_DOMAIN the smallest ordinal of a record with a sequence byte >= 0x80 */
    uint32_t seq_len;    /* the header's two bytes (0 without records): the last record's length ... */
    uint32_t packed_len; /* ... and its packed length, both modulo 256 */
} hpn_twobit_result;
int hpn_twobit_pack_begin(hpn_ctx *ctx, uint64_t max_bytes);
int hpn_twobit_pack_add(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, hpn_sort_info *info);
int hpn_twobit_pack_finish(hpn_ctx *ctx, hpn_twobit_result *result);
int hpn_twobit_pack_write(hpn_ctx *ctx, uint64_t offset, void *out, uint64_t cap, uint64_t *written);
int hpn_twobit_unpack(hpn_ctx *ctx, uint32_t seq_len, uint32_t packed_len, const void *packed, uint64_t n_records, void *out, uint64_t out_cap,
                      uint64_t *out_bytes);

/* ---- pick_pair.c: two FASTQ files split into the reads that still have a mate and those that do not ----------
 * pick_pair frames both streams as readNextNode frames them (see above; here the quality line KEEPS its line end, so a last line
 * without '\n' goes out without one) and walks them against each other with c(a, b) = strncmp(a.name, b.name, k), k the offset
 * of the first space in A's name (a name without one is compared whole):
 *     loop: a = next(A); b = next(B)
 *           while a && c(a, b) < 0:  a -> 1_SE; a = next(A)
 *           while b && c(a, b) > 0:  b -> 2_SE; b = next(B)
 *           if !a && !b: stop
 *           a -> 1_PE; b -> 2_PE
 * An output record is "name\nsequence\n+\nquality line".  The walk is no clean merge-join (each while runs once per round, so it
 * can pair different names), and it dereferences a NULL record when one file runs out in front of the other.  The device does
 * not walk: it PROPOSES a pairing and VERIFIES, record by record, that the walk produces exactly that one
 * (docs/kernels/fastq_pair.md) -- first the identity, when both files hold the same number of records, then a join that takes
 * file B for ascending.  What verifies is exact for any input, sorted or not; what does not is left to the caller.
 *
 *   hpn_fastq_pair_begin   opens a session (closing the context's earlier one).  max_bytes: as for hpn_fastq_uniq_begin, both
 *                          mates' text together.
 *   hpn_fastq_pair_add     one chunk of mate 0 (READ1) or 1 (READ2), the chunk contract of hpn_fastq_sort_add (the same framing,
 *                          the same info); the mates may be fed in any interleaving.  Irregular text -- HPN_TEXT_NUL, _LONG_LINE,
 *                          _PARTIAL, _DENSE -- is reported in info->irregular and closes the session.  HPN_E_CAPACITY and
 *                          HPN_E_DOMAIN (2^31 or more records) as there.
 *   hpn_fastq_pair_finish  after both mates' last chunks: proposes, verifies, writes the four texts on the device, fills
 *                          *result.  When neither proposal verifies: HPN_E_DOMAIN, result->unverified is 1, fail_mate and
 *                          fail_record name the first record of the join's proposal that the walk treats otherwise, there are no
 *                          outputs and the session is closed -- the device has no answer, the reference may have one.
 *   hpn_fastq_pair_write   copies up to `cap` bytes of output `which_output` (HPN_PAIR_OUT_*; result->out_bytes[which_output]
 *                          in all), from byte `offset` on, to `out` (host or device). */
#define HPN_PAIR_IDENTITY 0u /* route: record i of READ1 with record i of READ2 */
#define HPN_PAIR_JOIN 1u     /* route: the join over an ascending READ2 */
#define HPN_PAIR_OUT_1_PE 0
#define HPN_PAIR_OUT_1_SE 1
#define HPN_PAIR_OUT_2_PE 2
#define HPN_PAIR_OUT_2_SE 3
typedef struct hpn_pair_result {
    uint64_t n_records[2]; /* records of READ1, READ2 */
    uint64_t n_pairs;      /* records in _1_PE (and in _2_PE) */
    uint64_t n_single[2];  /* records in _1_SE, _2_SE */
    uint64_t out_bytes[4]; /* bytes of _1_PE, _1_SE, _2_PE, _2_SE */
    int64_t fail_record;   /* -1, or with unverified the 0-based ordinal of the first record that does not verify ... */
    uint32_t fail_mate;    /* ... and its file: 0 READ1, 1 READ2 */
    uint32_t route;        /* HPN_PAIR_IDENTITY or HPN_PAIR_JOIN: the proposal that verified (or the last one tried) */
    uint32_t unverified;   /* 1 with HPN_E_DOMAIN: neither proposal is what the walk produces */
    uint32_t reserved;
} hpn_pair_result;
int hpn_fastq_pair_begin(hpn_ctx *ctx, uint64_t max_bytes);
int hpn_fastq_pair_add(hpn_ctx *ctx, int mate, const void *text, uint64_t nbytes, int last, hpn_sort_info *info);
int hpn_fastq_pair_finish(hpn_ctx *ctx, hpn_pair_result *result);
int hpn_fastq_pair_write(hpn_ctx *ctx, int which_output, uint64_t offset, void *out, uint64_t cap, uint64_t *written);

/* ---- gzfastq_mrle.c: the quality lines run-length packed, and decoded again ---------------------------------
 * gzfastq_mrle frames a stream as readNextNode frames it (see above) and keeps the input's order.  Each quality line is encoded
 * by a two-pass run-length codec over the six symbols '#' 0, '/' 1, '7' 2, '<' 3, 'B' 4, 'F' 5: pass 1 sums per symbol, over
 * its maximal runs of length L, L - 2 - (L - 1) / 255; the first output byte has bit s set where that sum is positive; a run of
 * such a symbol becomes the symbol, (L - 1) / 255 bytes 0xFF and the byte L - 255 * ((L - 1) / 255) - 1, every other run its L
 * bytes.  An empty line is the flag byte alone; a line encodes to at most its length + 1 bytes.  Any other quality byte indexes
 * the reference's 8-entry table at 255: there is no answer.  Three outputs:
 *   HPN_MRLE_PACKED  per record (uint8_t)size and the `size` encoded bytes (the reference's PREFIX_sort_by_seq.fq);
 *   HPN_MRLE_TEXT    per record what the decoder makes of those encoded bytes and the line's length, and '\n' (its stdout);
 *   HPN_MRLE_SHARED  what one descriptor receives when the packed file IS standard output (a prefix that begins with '-'): two
 *                    stdio streams with 4,096-byte buffers, four calls per record -- the line, "\n", the length byte, the
 *                    encoded bytes; a stream writes its next 4,096 bytes when a non-empty call does not fit into what is left
 *                    of its buffer; at the end the packed stream's remainder follows and the text's remainder is lost.
 *
 *   hpn_mrle_begin   opens a session (closing the context's earlier one).  max_bytes: as for hpn_fastq_uniq_begin.
 *   hpn_mrle_add     one chunk, the chunk contract of hpn_fastq_sort_add (the same framing, the same info): irregular text --
 *                    HPN_TEXT_NUL, _LONG_LINE, _PARTIAL, _DENSE -- is reported in info->irregular and closes the session.
 *                    HPN_E_CAPACITY and HPN_E_DOMAIN (2^31 or more records) as there.
 *   hpn_mrle_finish  after the last chunk: encodes, decodes and lays out the shared stream on the device, fills *result.  A
 *                    quality byte outside the six: HPN_E_DOMAIN, result->bad_record is the smallest 0-based ordinal of such a
 *                    record and the session is closed.
 *   hpn_mrle_write   copies up to `cap` bytes of output `which` (HPN_MRLE_*; result->out_bytes[which] in all), from byte
 *                    `offset` on, to `out` (host or device). */
#define HPN_MRLE_PACKED 0
#define HPN_MRLE_TEXT 1
#define HPN_MRLE_SHARED 2
typedef struct hpn_mrle_result {
    uint64_t n_records;    /* records encoded */
    uint64_t out_bytes[3]; /* bytes of the packed, the text and the shared output */
    int64_t bad_record;    /* -1, or with HPN_E_DOMAIN the smallest ordinal of a record with a quality byte outside #/7<BF */
} hpn_mrle_result;
int hpn_mrle_begin(hpn_ctx *ctx, uint64_t max_bytes);
int hpn_mrle_add(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, hpn_sort_info *info);
int hpn_mrle_finish(hpn_ctx *ctx, hpn_mrle_result *result);
int hpn_mrle_write(hpn_ctx *ctx, int which, uint64_t offset, void *out, uint64_t cap, uint64_t *written);

/* ---- Rfastqc.R's one call: qsort_hash_count(fq1, fq2) of Rgzfastq_uniq.c, from FASTQ text ----------------------
 * The whole list the plugin returns -- 5 elements single-end, 9 paired -- from one or two streams framed as readNextNode frames
 * them (see hpn_fastq_sort_*).  With L1, L2 the sequence lengths of a record (a pair, ordinal by ordinal):
 *
 *   HPN_RFASTQC_DUP         int32[n_unique]   the count of every distinct KEY, descending (element 1).  The key is the C string the
 *                                             plugin assembles in a zeroed 512-byte buffer:
 *                                               single-end               s1[0:50] if L1 > 75, else s1
 *                                               L2 > 75,  L1 < 50        s1                   (a NUL gap cuts mate 2 off)
 *                                               L2 > 75,  L1 >= 50       s1[0:50] + s2[0:50]  (mate 2 overwrites s1[50:])
 *                                               L2 <= 75, L1 > 75        s1[0:50]             (mate 2 lies behind a NUL gap)
 *                                               L2 <= 75, L1 <= 75       s1 + s2              (no separator: AC/GT is ACG/T)
 *                                             compared bytewise.  Only the multiset of counts is defined (table and qsort order
 *                                             cannot be seen in it).
 *   HPN_RFASTQC_GC          double[n_records] #{'G','C'} / L per read of `mate` (elements 2, 6)
 *   HPN_RFASTQC_QUALITY     int32[128*300]    quality[q + 128*pos], over the QUALITY line's own length (elements 3, 7)
 *   HPN_RFASTQC_NUCLEOTIDE  int32[5*300]      nucleotide[5*pos + code], codes as for hpn_fastq_rqc (elements 4, 8)
 *   HPN_RFASTQC_LENGTH      int32[300]        length[L - 1] (elements 5, 9)
 *
 *   hpn_rfastqc_begin   opens a session (closing the context's earlier one).  paired, max_bytes, hash_bits: as for
 *                       hpn_fastq_uniq_begin (hash_bits 0: 64 bits; a small value makes clashes the rule, for tests -- the answer
 *                       never rests on the hash).
 *   hpn_rfastqc_add     one chunk of `mate` (0, or 1 in a paired session), the chunk contract and the info of hpn_fastq_sort_add;
 *                       the mates' streams may be fed in any interleaving.  Irregular text closes the session.  HPN_E_CAPACITY
 *                       and HPN_E_DOMAIN (2^31 or more records: the plugin's cells are int) as there.
 *   hpn_rfastqc_finish  after every mate's last chunk: tallies and groups on the device, fills *result.  Records of mate 2 behind
 *                       mate 1's last are ignored, as the plugin never reads them.  Where the plugin has no answer it returns
 *                       HPN_E_DOMAIN, names the first offending record and mate (in the plugin's order: per record mate 1, then
 *                       mate 2) with the reason, and closes the session with nothing to read:
 *                         HPN_RFASTQC_BAD_LENGTH   L outside 1..300 (it writes outside Length[] / the matrices)
 *                         HPN_RFASTQC_BAD_QUALITY  a quality line longer than 300
 *                         HPN_RFASTQC_BAD_BYTE     a sequence or quality byte >= 128 (a negative index through char)
 *                         HPN_RFASTQC_MATE_SHORT   mate 2 has fewer records than mate 1 (it dereferences NULL); bad_record is
 *                                                  mate 2's record count, bad_mate 1
 *   hpn_rfastqc_read    copies up to cap_elems ELEMENTS of array `which` of `mate` (mate is ignored for HPN_RFASTQC_DUP), from
 *                       element first_elem on, to `out` (host or device); *got: how many.  Call until *got is 0. */
#define HPN_RFASTQC_DUP 0
#define HPN_RFASTQC_GC 1
#define HPN_RFASTQC_QUALITY 2
#define HPN_RFASTQC_NUCLEOTIDE 3
#define HPN_RFASTQC_LENGTH 4
#define HPN_RFASTQC_BAD_LENGTH 1u
#define HPN_RFASTQC_BAD_QUALITY 2u
#define HPN_RFASTQC_BAD_BYTE 3u
#define HPN_RFASTQC_MATE_SHORT 4u
typedef struct hpn_rfastqc_result {
    uint64_t n_records;    /* records (pairs) tallied */
    uint64_t n_unique;     /* distinct keys: the length of HPN_RFASTQC_DUP */
    uint64_t hash_clashes; /* sorted neighbours with equal grouping hashes over different keys */
    int64_t bad_record;    /* -1, or with HPN_E_DOMAIN the 0-based ordinal of the first record the plugin has no answer for */
    uint32_t bad_mate;     /* ... and its mate (0, 1) */
    uint32_t reason;       /* 0, or HPN_RFASTQC_BAD_* / _MATE_SHORT */
} hpn_rfastqc_result;
int hpn_rfastqc_begin(hpn_ctx *ctx, int paired, uint64_t max_bytes, uint32_t hash_bits);
int hpn_rfastqc_add(hpn_ctx *ctx, int mate, const void *text, uint64_t nbytes, int last, hpn_sort_info *info);
int hpn_rfastqc_finish(hpn_ctx *ctx, hpn_rfastqc_result *result);
int hpn_rfastqc_read(hpn_ctx *ctx, int which, int mate, uint64_t first_elem, void *out, uint64_t cap_elems, uint64_t *got);

/* ---- map_kseq.cpp / kbtree_kseq.c: kseq input, the first record of every distinct sequence, in the sequences' order -----
 * The text is framed as the two programs' kseq_read frames it (klib/kseq.h over a kseq_t that is NEW for every record): a
 * header starts at the next '>' or '@' -- at ANY byte, because the new kseq_t has forgotten that the sequence loop consumed
 * the next header's first byte; the name runs to the first isspace byte; unless that byte is '\n' the rest of the line is the
 * comment (a trailing '\r' dropped when the comment is longer than one byte); sequence lines follow up to a line that starts
 * with '>', '+' or '@', empty lines skipped, after every appended line a trailing '\r' dropped when the accumulated length is
 * above 1; behind a '+' line quality lines are appended until they reach the sequence's length.  The device frames two shapes:
 *
 *   FASTQ  four lines per record and a line count divisible by 4: line 0 starts with '@', line 1 is not empty and does not
 *          start with '>', '+' or '@', line 2 starts with '+', line 3 has line 1's length (both after the '\r' rule).
 *   FASTA  the stream's first byte is '>', no line starts with '@' or '+', the last line is no header without its '\n'.
 *          Every line that starts with '>' opens a block.  kseq_read, coming from a FASTA record, looks for the next '>' or
 *          '@' behind the first byte of the NEXT block: the blocks 0, 2, 4, ... are the records, and a block 1, 3, 5, ... that
 *          holds a '>' or '@' behind its first byte is not regular.
 *   In both: no NUL byte, no header line, joined sequence or "name comment" beyond 65,535 bytes.
 *
 * Anything else -- wrapped FASTQ, mixed '>' and '@' records, a truncated tail, text in front of the first header -- is
 * reported as HPN_TEXT_KSEQ in info->irregular and closes the session (host/kseq_read.hpp reads such text on the host).
 * Records are copied into a normalised store as "name comment\nsequence\n[quality]" with "(null)" where the programs print a
 * NULL comment, ordered by the sequence's bytes as unsigned (a prefix first: strcmp on text without NUL) with equal ones in
 * input order, and the first of every run of equal sequences is written as "name comment\nseq\n+\nqual\n", "(null)" for the
 * quality a FASTA record does not have.
 *
 *   hpn_kseq_begin   opens a session (closing the context's earlier one and releasing its arrays, the ordering's included).  max_bytes: as for hpn_fastq_uniq_begin.
 *   hpn_kseq_add     one chunk, cut anywhere (inside a header, between the lines of a wrapped sequence, behind a '\r'); host or
 *                    device pointer; `last` closes the stream.  The unfinished record stays unframed until more bytes or
 *                    `last` arrive; one that has already joined more than 65,535 bytes, or an unframed span of 2^31 - 4 KiB bytes,
 *                    is HPN_TEXT_KSEQ at once.  A chunk the framing has no memory for closes the session (HPN_E_NOMEM).
 *                    HPN_E_CAPACITY and HPN_E_DOMAIN (2^31 or more records) as for hpn_fastq_uniq_add.
 *   hpn_kseq_finish  after the last chunk: orders, picks every run's first record, formats; fills *result.
 *   hpn_kseq_write   copies up to `cap` bytes of the output (result->out_bytes in all), from byte `offset` on, to `out`. */
#define HPN_KSEQ_NONE 0u  /* no byte seen */
#define HPN_KSEQ_FASTA 1u
#define HPN_KSEQ_FASTQ 2u
typedef struct hpn_kseq_result {
    uint64_t n_records;  /* records read */
    uint64_t n_distinct; /* distinct sequences: what the programs write to stderr */
    uint64_t out_bytes;  /* bytes of the output */
    uint64_t refined;    /* records that went through refinement rounds, summed over the rounds */
    uint32_t rounds;     /* radix rounds of the ordering (1: the first 6 bytes decided everything) */
    uint32_t shape;      /* HPN_KSEQ_* */
    uint32_t one_length; /* 1: every sequence has one length (or there is none) */
    uint32_t first_len;  /* the first record's sequence length, and ... */
    uint32_t other_len;  /* ... with one_length 0, the length of the first record that differs from it */
    uint32_t reserved;
} hpn_kseq_result;
int hpn_kseq_begin(hpn_ctx *ctx, uint64_t max_bytes);
int hpn_kseq_add(hpn_ctx *ctx, const void *text, uint64_t nbytes, int last, hpn_sort_info *info);
int hpn_kseq_finish(hpn_ctx *ctx, hpn_kseq_result *result);
int hpn_kseq_write(hpn_ctx *ctx, uint64_t offset, void *out, uint64_t cap, uint64_t *written);

/* ---- ONE text stream framed by several contexts (one per GPU): pieces ----------------------------
 * Record-block sharding of a single FASTQ input (the reference's parallelism stops at
 * whole files, fastq_count.c:213-230, klib/kthread.c:34-60).  The stream's bytes T[0, N) are cut at
 * arbitrary positions 0 = b_0 < b_1 < ... into pieces [b_j, b_j+1).  A piece OWNS the records whose
 * first byte lies in it.  Which lines start a record depends on how many lines the stream has before
 * the piece, so a piece is framed in two steps, each on the context that holds it:
 *
 *   hpn_fastq_text_piece_lines   text = T[b_j - head, b_j+1 + tail): `head` = 1 byte in front of the
 *       piece (0 for the stream's first piece), own_bytes = b_j+1 - b_j, and a tail of the following
 *       bytes -- 4096 hold the rest of any regular record that starts in the piece (fewer only where the
 *       stream ends); last != 0: the piece ends the stream (no tail).  Copies, indexes the lines and
 *       returns out->n_lines = number of '\n' in T[b_j - head, b_j+1 - 1): the n_lines of pieces
 *       0 .. j-1 add up to the lines in front of piece j's text -- the only thing pieces tell each other.
 *   hpn_fastq_text_piece_count / _trim   lines_before = that sum.  Frames the records the piece owns
 *       and tallies / trims them exactly like hpn_fastq_text_count / _trim do for a chunk.
 *
 * Irregular text (same conditions; a record that does not end inside the tail counts as a long line)
 * is reported in ->irregular by either call and nothing is added: the caller frames the WHOLE stream
 * another way.  No bytes are carried between pieces, so different contexts may work on different
 * pieces at the same time; one context handles one piece at a time. */
typedef struct hpn_text_piece {
    uint64_t n_lines;
    uint32_t irregular; /* HPN_TEXT_* reasons visible without record framing (NUL, DENSE) */
    uint32_t reserved;
} hpn_text_piece;
#define HPN_TEXT_PIECE_TAIL 4096u
int hpn_fastq_text_piece_lines(hpn_ctx *ctx, const void *text, uint64_t nbytes, uint32_t head, uint64_t own_bytes,
                               int last, hpn_text_piece *out);
int hpn_fastq_text_piece_count(hpn_ctx *ctx, uint64_t lines_before, uint32_t tally_flags, hpn_text_info *info);
int hpn_fastq_text_piece_trim(hpn_ctx *ctx, uint64_t lines_before, int32_t S, int32_t E, void *out_text,
                              uint64_t out_cap, hpn_text_info *info);

/* ---- BGZF: inflate on the device ------------------------------------------------------------
 * A BAM / bgzip file is a chain of independent gzip members of at most 64 KiB (SAM spec 4.1);
 * the reference inflates them one by one on the host (samtools-0.1.19 bgzf.c:214-307).  Here
 * the host only walks the 18-byte block headers; every block is decoded by one wavefront.
 * blocks[i]: in_off / in_len = the raw DEFLATE payload inside the compressed buffer (after the
 * member header, before the 8-byte trailer), out_off / out_len = where its ISIZE bytes go.
 * d_comp must be readable 64 bytes past the last payload.  d_status[i] = 0 or a decoder error
 * code (malformed stream, or output != out_len); like the reference's reader the CRC32 is not
 * checked.  Asynchronous on the context's stream. */
typedef struct hpn_bgzf_block {
    uint64_t in_off;
    uint32_t in_len, out_len;
    uint64_t out_off;
} hpn_bgzf_block;
int hpn_bgzf_inflate_dev(hpn_ctx *ctx, const uint8_t *d_comp, const hpn_bgzf_block *d_blocks, uint64_t n_blocks,
                         uint8_t *d_out, uint32_t *d_status);

/* ---- one gzip member inflated on the device (two passes) -------------------------------------
 * gzread behind the 4 x gzgets loops (fastq_count.c:112-118, IO_stream.h:122-136) on a single-
 * member .fastq.gz: one DEFLATE stream, every byte of which may refer to the 32 KiB before it.
 * The host cuts the stream into stretches that start at deflate block boundaries (it finds them,
 * csrc/host/pgz_reader.hpp find_start); here every stretch is inflated by one wavefront with the
 * history unknown (16-bit symbols, placeholders for history bytes), the histories are resolved in
 * stream order, and the symbols are translated into one contiguous text.
 * chunks[i]: in_off = byte of d_comp holding the stretch's first bit, start_bit = 0..7, in_len =
 * bytes readable from in_off (d_comp must be readable 64 bytes beyond), end_bit = where the
 * stretch must end in bits from in_off * 8 (the next stretch's first bit), ~0 for "at the final
 * block".  A stretch that does not end exactly there on a block boundary is an error: that is what
 * proves every start.  sym_cap (multiple of 8) = symbols of scratch per stretch; n_chunks <= 65535.
 * d_window_in / d_window_out (32768 bytes, may be NULL): the history before the first stretch /
 * after the last, for streams inflated in several calls.  info: n_bytes = text produced (if it
 * exceeds text_cap: HPN_E_CAPACITY, nothing written), status = 0 or the first failing stretch's
 * decoder code (bad_chunk says which), final_chunk = 1 + index of the stretch that ended at a
 * final block (0: none), end_bit = bit position that stretch reached (the member trailer).
 * Synchronous.  CRC-32 is not checked (ISIZE is the caller's to check).  in_len < 2^31.
 * status codes: 1-11 malformed block header or code tables, 12/14 out of symbol scratch (sym_cap), 13/15 invalid
 * code in the data, 17 ran past in_len, 20 the stretch did not end on end_bit at a block boundary, 22 a final block
 * inside a stretch that was given an end and nothing that starts another member behind it (the next stretch's start is
 * unproven), 23 more members ended inside the call than it has room for (65536), 24 a header too long to back out of,
 * 25 a match that reaches in front of the stream's first byte (d_window_in NULL: the call starts the stream).
 *
 * Several members (cat a.gz b.gz): a stretch that meets a final block looks behind the 8-byte trailer for the next
 * member's header (RFC 1952) and goes on with its first block.  hpn_gz_members() lists the members that ended inside the
 * last call -- text_end = bytes of the call's text up to the member's end, isize = the ISIZE field of its trailer -- in
 * text order, so that the caller can check every member's size; the last member of the file ends the last stretch
 * (hpn_gz_info.final_chunk, .end_bit) as a single member does. */
typedef struct hpn_gz_chunk {
    uint64_t in_off;
    uint64_t end_bit;
    uint32_t in_len;
    uint32_t start_bit;
} hpn_gz_chunk;
typedef struct hpn_gz_info {
    uint64_t n_bytes;
    uint64_t end_bit;
    uint32_t status, bad_chunk, final_chunk, reserved;
} hpn_gz_info;
typedef struct hpn_gz_member {
    uint64_t text_end;
    uint32_t isize, crc32; /* the two fields of the member's trailer (RFC 1952) */
} hpn_gz_member;
int hpn_gz_inflate_dev(hpn_ctx *ctx, const uint8_t *d_comp, const hpn_gz_chunk *d_chunks, uint32_t n_chunks,
                       uint32_t sym_cap, const uint8_t *d_window_in, uint8_t *d_text, uint64_t text_cap,
                       uint8_t *d_window_out, hpn_gz_info *info);
int hpn_gz_members(hpn_ctx *ctx, hpn_gz_member *out, uint32_t cap, uint32_t *n); /* HPN_E_CAPACITY: *n tells how many */
/* Decoder wavefronts the context's device runs at once (CUs x decoders per CU): one stretch (hpn_gz_inflate_dev) or one BGZF
 * block (hpn_bgzf_inflate_dev) each -- the number of stretches that fills the chip exactly once.  Hosts size their batches by it. */
int hpn_inflate_slots(hpn_ctx *ctx, uint32_t *n_slots);
/* The same call in two halves, for ONE file whose batches of stretches go to several contexts (one per GPU) in turn: the
 * symbolic decode of a batch needs nothing of the text in front of it, only the resolution of the histories does (the 32 KiB
 * window the batch before ends with).  _begin_dev starts the decode on the context's stream and returns; _finish_dev takes the
 * window (d_window_in: on THIS context's device; NULL for the file's first batch), resolves, translates into d_text and
 * reports like hpn_gz_inflate_dev; d_window_out receives this batch's last 32 KiB for the next one (the caller carries it
 * to the next context's device).  HPN_E_CAPACITY from _finish_dev leaves the decoded symbols in place: call it again with
 * the room info->n_bytes asks for.  hpn_gz_inflate_dev = _begin_dev + _finish_dev.  gzread behind the reference's gzgets
 * (IO_stream.h:122-136, fastq_count.c:112-118) is what the pair stands in for. */
int hpn_gz_inflate_begin_dev(hpn_ctx *ctx, const uint8_t *d_comp, const hpn_gz_chunk *d_chunks, uint32_t n_chunks, uint32_t sym_cap);
int hpn_gz_inflate_finish_dev(hpn_ctx *ctx, const uint8_t *d_window_in, uint8_t *d_text, uint64_t text_cap, uint8_t *d_window_out,
                              hpn_gz_info *info);

/* CRC-32 (RFC 1952) of byte ranges of a device buffer: crc[k] of d_data[spans[k].off .. + spans[k].len).  gzread, which the
 * reference reads every input through (IO_stream.h:122-136), verifies each gzip member's CRC-32 and stops handing out bytes
 * where one fails; a member inflated on the device is verified with this (in pieces, as the text comes: hpn_crc32_join folds
 * CRC(A), CRC(B), |B| into CRC(A || B)).  spans and crc are host arrays.  Synchronous. */
typedef struct hpn_span {
    uint64_t off, len;
} hpn_span;
int hpn_crc32_dev(hpn_ctx *ctx, const uint8_t *d_data, const hpn_span *spans, uint32_t n_spans, uint32_t *crc);
uint32_t hpn_crc32_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* Where deflate blocks start, by trial, on the device: found[k] = the first bit position in [slices[k].off, slices[k].off +
 * slices[k].len) (bits, from d_comp) at which a non-final dynamic-Huffman block decodes to text and something that begins
 * like a block follows, or ~0.  What the host's gz_find_block_start does on the cores (csrc/host/pgz_reader.hpp); a start
 * found here is a proposal like one found there: it is proven by the stretch before it arriving exactly there
 * (hpn_gz_inflate_dev, status 20 otherwise).  d_comp: comp_bytes bytes, readable for 256 more.  slices / found: host
 * arrays.  Synchronous. */
int hpn_gz_find_starts_dev(hpn_ctx *ctx, const uint8_t *d_comp, uint64_t comp_bytes, const hpn_span *slices, uint32_t n,
                           uint64_t *found);

/* ---- BAM record batches ---------------------------------------------------------------
 * What the reference's bam_fetch_f callback sees per record (bam.h:178-187,627),
 * flattened to SoA by the host decoder: core fields, CIGAR words (len<<4|op,
 * bam.h:97-110) and the 4-bit packed sequence (bam.h:260). */
typedef struct hpn_bam_batch {
    uint64_t n;
    const int32_t *tid;
    const int32_t *pos;
    const uint32_t *flag;
    const int32_t *l_qseq;
    const uint32_t *cigar_off; /* [n+1] into cigar */
    const uint32_t *cigar;
    const uint64_t *seq_off;   /* [n+1] into seq4 (bytes); may be NULL for depth */
    const uint8_t *seq4;       /* may be NULL for depth */
} hpn_bam_batch;

/* ---- bam2depth: replaces fetch_func + hash2BedGraph + overlap ----------------------
 * bam2depth.c:86-110 (CIGAR-M difference array), :203-236 (sorted sweep -> runs of
 * equal depth > 0), :132-176 (window sums).  One target (chromosome) at a time:
 *   hpn_depth_begin(tid, target_len, flag_mask)   flag_mask = 0x704 for bam2depth
 *                                                 (BAM_DEF_MASK, bam.h:124), 0x4 for bam2wig
 *   hpn_depth_add(batch)            any number of times; records of other tids are skipped
 *   hpn_depth_finish(W, ...)        runs (start,end,depth) ascending + per-window sum of coverage
 * win_sum has target_len/W+1 entries (bam2depth.c:326) holding the exact integer
 * sum of coverage over [kW, min((k+1)W, target_len)); the host prints win_sum/W
 * with %.2f (output_bins :238-246).
 * Domain: every breakpoint < 2^28 (int2char keeps 28 bits, hashtbl.c:243-249). */
typedef struct hpn_run {
    int32_t start, end, depth;
} hpn_run;

int hpn_depth_begin(hpn_ctx *ctx, int32_t tid, uint32_t target_len, uint32_t flag_mask);
/* The same, telling the window size hpn_depth_finish will be called with.  A BAM that bam2depth can read is coordinate-
 * sorted (it needs the index, bam2depth.c:112-119), and on sorted input the work is done WHILE the records come: every
 * stretch of the target that the records of an hpn_depth_add call have moved beyond is swept at once -- prefix sum, runs,
 * window sums, in the workgroup that gathered its breakpoints -- and never goes through memory as a difference array.
 * Window sums can only ride along if W is known by then; with W = 0 (hpn_depth_begin) or another W at hpn_depth_finish
 * they are taken from the runs afterwards (same numbers, one more pass over the runs).
 * This expects the records of the target in coordinate order ACROSS calls (inside a call any order is handled).  A record
 * that arrives behind positions already swept makes hpn_depth_finish fail with HPN_E_STATE; callers with input in any
 * order put HPN_DEPTH_ANY_ORDER into flag_mask: nothing is swept early then. */
#define HPN_DEPTH_ANY_ORDER 0x80000000u
int hpn_depth_begin_w(hpn_ctx *ctx, int32_t tid, uint32_t target_len, uint32_t flag_mask, uint32_t W);
/* How far the target has been swept by the hpn_depth_add calls so far: positions [0, *swept_positions) are final (waits for the
 * calls' kernels).  0 with HPN_DEPTH_ANY_ORDER, or while no batch could be taken that way. */
int hpn_depth_progress(hpn_ctx *ctx, uint64_t *swept_positions);
int hpn_depth_add(hpn_ctx *ctx, const hpn_bam_batch *host_batch);
int hpn_depth_add_dev(hpn_ctx *ctx, const hpn_bam_batch *dev_batch);
/* runs: caller buffer of runs_cap entries; *n_runs receives the number found
 * (HPN_E_CAPACITY if it exceeds runs_cap; call again with a larger buffer --
 * the scan result stays valid until the next hpn_depth_begin). */
/* (runs == NULL with runs_cap == 0: the runs stay on the device, *n_runs is still set -- for callers that
 * take the bedGraph text instead, below.) */
int hpn_depth_finish(hpn_ctx *ctx, uint32_t W, hpn_run *runs, uint64_t runs_cap, uint64_t *n_runs,
                     uint64_t *win_sum);
/* hash2BedGraph's fprintf(bedGraph, "%s\t%d\t%d\t%d\n", chr, start, end, depth) (bam2depth.c:217) for every
 * run of the last hpn_depth_finish, formatted on the device: *n_bytes = size of the text, which stays on
 * the device until the next hpn_depth_begin / hpn_depth_bedgraph_format; hpn_depth_bedgraph_read copies
 * text[offset, offset + nbytes) to `dst` (host; pinned memory makes the copy faster). */
int hpn_depth_bedgraph_format(hpn_ctx *ctx, const char *target_name, uint64_t *n_bytes);
int hpn_depth_bedgraph_read(hpn_ctx *ctx, uint64_t offset, void *dst, uint64_t nbytes);
/* Where the text of the last hpn_depth_bedgraph_format lies on the device, for a caller that copies it out itself -- through
 * another context's stream (hpn_memcpy_d2h), beside the kernels of the NEXT target: the bytes stay put until this context's
 * next hpn_depth_bedgraph_format (hpn_depth_begin / _add / _finish do not touch them).  bam2depth's writer does this. */
int hpn_depth_bedgraph_dev(hpn_ctx *ctx, const uint8_t **d_text, uint64_t *n_bytes);

/* ---- bam_sliding_count: replaces fetch_func + cal_GC ----------------------------------
 * bam_sliding_count.c:84-124.  Slot of a record = win_off[tid] + (uint16)(pos/W)
 * (:117, including the 16-bit wrap).  Adds per slot: bins += 1, gc += #nibbles
 * equal to 2 (C) or 4 (G), len += l_qseq; sets touched[tid].  Records with tid<0
 * or flag&4 are skipped (:96-97).  All integer; the float32 replay of
 * calc_winGC (:126-138) is host work (csrc/host/report.cpp). */
int hpn_window_begin(hpn_ctx *ctx, int32_t n_targets, const uint64_t *win_off /*[n_targets+1]*/,
                     uint32_t W);
int hpn_window_add(hpn_ctx *ctx, const hpn_bam_batch *host_batch);
int hpn_window_add_dev(hpn_ctx *ctx, const hpn_bam_batch *dev_batch);
int hpn_window_finish(hpn_ctx *ctx, uint32_t *bins, uint64_t *gc, uint32_t *len, uint8_t *touched,
                      uint64_t *n_count);

/* ---- BAM records in place in inflated BGZF blocks -----------------------------------------
 * bam_read1 (samtools-0.1.19 bam.c:191) on the device: after hpn_bgzf_inflate_dev the records
 * are indexed where they lie.  The inflated blocks of a call are ONE stream d_raw[0, out_off + out_len
 * of the last block): `first_off` is the stream offset of its first record (inside block 0: the block
 * the BAM header ends in; 0 when the caller has put the unfinished record of the call before in front,
 * see tail_bytes).  Where every block's first record starts is found on the device and proven for the
 * whole call (every block's chain must arrive exactly at the next block's found start: by induction
 * from first_off all starts are true), so both writers' files decode: samtools never lets a record
 * straddle a block (bam.c:238 bgzf_flush_try), htsjdk packs records across blocks -- which bgzf_read
 * (bgzf.c:342) hides from the reference.  info->flags: 1 = the proof failed or a record is impossible
 * (a damaged file, or records longer than a block), 2 = a block failed to inflate -- in both cases
 * nothing is indexed and the caller decodes the file on the host; 4 (informational) = records do run
 * across block ends.  info->tail_bytes: the call's stream ends inside a record of which that many bytes
 * are there (not indexed): the caller copies d_raw[stream end - tail_bytes, stream end) in front of the
 * next call's stream (out_off of its blocks moved up by as much) and passes first_off = 0.
 * Synchronous (returns the record count and the refID range of the batch).  The two add calls then run
 * the depth / window kernels over the indexed records, like hpn_depth_add_dev / hpn_window_add_dev.
 * d_raw must be readable 16 bytes past the end of the inflated stream (the window kernel
 * reads packed sequences in unaligned 16-byte pieces). */
typedef struct hpn_raw_info {
    uint64_t n_records;
    int32_t tid_min, tid_max;
    uint32_t flags, tail_bytes;
} hpn_raw_info;
int hpn_bam_raw_index_dev(hpn_ctx *ctx, const uint8_t *d_raw, const hpn_bgzf_block *d_blocks, uint64_t n_blocks,
                          uint32_t first_off, const uint32_t *d_status, hpn_raw_info *info);
int hpn_depth_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw);
int hpn_window_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw);

/* ---- bamSplitChr: one BAM per target, cut into BGZF blocks as samtools' writer cuts them ------
 * bamSplitChr.c:129-138 -- bam_fetch(tid, 0, 1 << 29) + samwrite per target -- for a coordinate-sorted file: a target's
 * records are one slice of the inflated stream, copied verbatim (4 + block_size bytes each) and cut by bam_write1's rule
 * (bam.c:238 bgzf_flush_try, bgzf.c bgzf_write): with `off` the fill of the open block and s the record's size, the block is
 * closed first if off + s > 0xff00, the record is appended, and a block that reaches 0xff00 is closed at once -- so a record
 * of 0xff00 bytes or more runs through blocks of exactly 0xff00.  A target's last block is closed when the target ends.
 *   hpn_bam_split_begin(n_ref, level0)
 *   per batch: hpn_bam_raw_index_dev(...), then hpn_bam_split_add_raw_dev(d_raw, last, &info)
 *              d_raw NULL: no records, only `last` (closes the open block at the end of the file)
 *   hpn_bam_split_blocks / _payload_dev / _stored_dev    what the call closed
 *   hpn_bam_split_finish                                  per-target record counts
 * The closed blocks of a call are listed in file order: off / len = the block's bytes inside the payload buffer
 * (hpn_bam_split_payload_dev; it holds the bytes of the block left open before in front of the batch's records), crc = their
 * CRC-32, tid = the target.  A target's last block of a call stays open (unless `last`): its bytes are kept on the device and
 * the next call's cuts start from its fill.  With level0 != 0 every closed block is also framed on the device as BGZF holding
 * one stored deflate block (len + 31 bytes: what deflate() makes of it at level 0), one after the other in list order:
 * hpn_bam_split_stored_dev.  Both buffers are valid until the next hpn_bam_split_* call.
 * Domain (outside it the reference's answer depends on the index's chunk lists): refID never decreases, with -1 behind every
 * placed record; pos never decreases inside a target; 0 <= pos < 2^29 and refID < n_ref for placed records.  The first
 * offending record since _begin is reported -- bad_record (ordinal, -1: none), bad_tid, bad_pos, reason (1 refID out of
 * range, 2 pos out of range, 3 refID goes backwards, 4 pos goes backwards) -- and the session makes no more blocks.
 * Synchronous. */
typedef struct hpn_split_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t n_blocks;       /* blocks this call closed */
    uint64_t payload_bytes;  /* bytes of the payload buffer the closed blocks cover (they lie in [0, payload_bytes)) */
    uint64_t stored_bytes;   /* size of the stored image (0 unless level0) */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    int32_t tid_first, tid_last; /* targets of the first and last closed block (0, -1: none) */
    uint32_t reason, open_bytes; /* open_bytes: fill of the block left open */
} hpn_split_info;
typedef struct hpn_split_block {
    uint64_t off;
    uint32_t len, crc;
    int32_t tid;
    uint32_t reserved;
} hpn_split_block;
typedef struct hpn_split_result {
    uint64_t n_records, n_blocks; /* since _begin */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, n_ref;
} hpn_split_result;
/* The framing on its own, for any producer of BGZF: spans[k] (host array) = len bytes (1 .. 0xff00) of d_data at off with
 * CRC-32 crc -> the block's len + 31 bytes at d_image + img_off.  Nothing outside a block's own image is written.  Synchronous. */
typedef struct hpn_stored_span {
    uint64_t off, img_off;
    uint32_t len, crc;
} hpn_stored_span;
int hpn_bgzf_stored_dev(hpn_ctx *ctx, const uint8_t *d_data, const hpn_stored_span *spans, uint32_t n_spans, uint8_t *d_image);
int hpn_bam_split_begin(hpn_ctx *ctx, int32_t n_ref, int level0);
int hpn_bam_split_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, int last, hpn_split_info *info);
int hpn_bam_split_blocks(hpn_ctx *ctx, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n); /* *n: blocks of the call from `first` on; HPN_E_CAPACITY if more than cap */
int hpn_bam_split_payload_dev(hpn_ctx *ctx, const uint8_t **d_payload, uint64_t *n_bytes);
int hpn_bam_split_stored_dev(hpn_ctx *ctx, const uint8_t **d_image, uint64_t *n_bytes);
int hpn_bam_split_finish(hpn_ctx *ctx, hpn_split_result *res, uint64_t *counts /* [n_ref] records per target, may be NULL */);

/* ---- samtools index: the .bai of a coordinate-sorted BAM ---------------------------------------
 * bam_index.c (samtools-0.1.19): bam_index_core's pass over the records on the device -- every record's virtual offset, the
 * runs of equal (refID, stored bin) that become chunks, the linear index, the per-target counts of the metadata bin 37450 --
 * and merge_chunks / fill_missing behind it.  (docs/kernels/bam_bai.md)
 *   hpn_bam_bai_begin(n_ref, target_len, first_voffset)      first_voffset: bam_tell behind the header
 *   per batch: hpn_bam_raw_index_dev(...), then hpn_bam_bai_add_raw_dev(d_raw, d_blocks, n_blocks, block_addr, last,
 *              end_voffset, &info) with the SAME block table (out_off as the record index saw it: moved up by the bytes of a
 *              carried record) and block_addr[0 .. n_blocks] (host) = the blocks' offsets in the file and the offset behind
 *              the last one.  A record's start is the end of the record before it, across calls; the end of a record whose
 *              last byte lies in block k is block_addr[k] << 16 | bytes into the block, and block_addr[k + 1] << 16 where it
 *              ends with the block.  d_raw NULL: no records.  last != 0 ends the file: end_voffset is what bam_tell says
 *              behind the failed read at the end of the file (file size << 16 for a file that ends with its data or with
 *              one empty block).
 *   hpn_bam_bai_finish(&res), hpn_bam_bai_read(targets, chunks, windows)
 * Results: per target (hpn_bai_target) the metadata -- off_beg / off_end, n_mapped / n_unmapped (flag & 4), has_records --,
 * its merged chunks chunks[first_chunk, + n_chunks) sorted by bin and, inside a bin, in file order, and its linear index
 * windows[first_window, + n_windows) with empty windows filled from the left (n_windows is set by the target's LAST mapped
 * record, not the largest).  The metadata bin is not among the chunks.
 * Domain: refID in [-1, n_ref) and never decreasing, -1 behind every placed record; pos >= 0 and never decreasing inside a
 * target; every mapped record's last window within (target_len - 1) >> 14; no CIGAR operation `B`; no stored bin 37450.  (A block of
 * no bytes ends the stream for samtools' reader: the caller hands none over except as the file's last.)  The first offending record since _begin is reported -- bad_record (ordinal, -1: none), bad_tid,
 * bad_pos, reason (1 refID out of range, 2 pos negative, 3 refID goes backwards, 4 pos goes backwards, 5 window beyond the
 * target, 6 CIGAR `B`, 7 stored bin 37450, 8 name and CIGAR do not fit the record, 9 more than 2^27 runs: bad_record is then the
 * first record of the batch that went over) -- and the session makes nothing more: the caller indexes the file on the host
 * (csrc/host/bai_build.hpp), which follows the reference everywhere.  Synchronous. */
typedef struct hpn_bai_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t n_runs;         /* runs of equal (refID, bin) that start in this batch */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_bai_info;
typedef struct hpn_bai_chunk {
    uint64_t beg, end;       /* virtual offsets */
    uint32_t bin;
    int32_t tid;
} hpn_bai_chunk;
typedef struct hpn_bai_target {
    uint64_t off_beg, off_end, n_mapped, n_unmapped;
    uint64_t first_chunk, n_chunks, first_window;
    int32_t n_windows;
    uint32_t has_records;
} hpn_bai_target;
typedef struct hpn_bai_result {
    uint64_t n_records, n_chunks, n_windows, n_no_coor; /* since _begin; n_chunks, n_windows: entries hpn_bam_bai_read fills */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, n_ref;
} hpn_bai_result;
int hpn_bam_bai_begin(hpn_ctx *ctx, int32_t n_ref, const int32_t *target_len, uint64_t first_voffset);
int hpn_bam_bai_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, const hpn_bgzf_block *d_blocks, uint64_t n_blocks, const uint64_t *block_addr,
                            int last, uint64_t end_voffset, hpn_bai_info *info);
int hpn_bam_bai_finish(hpn_ctx *ctx, hpn_bai_result *res);
int hpn_bam_bai_read(hpn_ctx *ctx, hpn_bai_target *targets /* [n_ref] */, hpn_bai_chunk *chunks /* [n_chunks] */, uint64_t *windows /* [n_windows] */);

/* ---- samtools sort: a BAM in coordinate order --------------------------------------------------
 * bam_sort.c (samtools-0.1.19) for the order by coordinate: the key of bam1_lt, (uint64_t)refID << 32 | (pos + 1) << 1 | strand
 * (strand: flag 0x10), sorted stably -- records of one key keep their input order, refID -1 goes last, any other refID sorts by
 * its unsigned value --, and the sorted records cut into BGZF blocks by bam_write1's rule (see hpn_bam_split_*).
 * (docs/kernels/bam_sort.md)
 *   hpn_bam_sort_begin()
 *   per batch: hpn_bam_raw_index_dev(...), then hpn_bam_sort_add_raw_dev(d_raw, &info): the batch's records are copied into
 *              the session's record store on the device (d_raw may be reused afterwards); d_raw NULL: no records
 *   hpn_bam_sort_finish(&res)             sorts; res.payload_bytes: the records' bytes, res.fresh_mem: what bam_sort_core_ext
 *                                         would have counted if every record had come into a fresh slot, the sum of
 *                                         72 + kroundup32(block_size - 32) -- below max_mem the reference sorts in one block
 *   hpn_bam_sort_order(order, n)          order[j]: the input ordinal of the j-th record of the output (n = res.n_records)
 *   hpn_bam_sort_sizes(sizes, n)          sizes[i] = 4 + block_size of input record i (the reference's chunk accounting)
 *   hpn_bam_sort_emit(first_record, max_records, last, &info)
 *              the next slice of the output, records [first_record, first_record + max_records) of the sorted order (slices
 *              are taken front to back: first_record is where the slice before ended): gathered behind the bytes of the block
 *              the slice before left open, cut, every closed block with its CRC-32.  The last block of a slice stays open
 *              unless `last` (which must come with the slice that takes the last record, or with an empty one behind it).
 *              info as in hpn_bam_split_add_raw_dev; every block's tid is 0.
 *   hpn_bam_sort_blocks / _payload_dev / _stored_dev    the slice's closed blocks, the payload buffer they point into, and
 *              (made when asked for) the blocks framed as stored BGZF blocks; valid until the next hpn_bam_sort_* call.
 * Domain: -1 <= pos <= 2^30 - 2 for every record (outside it bam1_lt's key and the key of the reference's merge step
 * disagree, and the order depends on the reference's chunking) and fewer than 2^31 records.  The first record outside it is
 * reported -- bad_record (ordinal, -1: none), bad_tid, bad_pos, reason (1 pos below -1, 2 pos above 2^30 - 2, 3 the 2^31-th
 * record) -- and nothing is sorted: the caller sorts on the host (csrc/host/bam_sort_host.hpp).  Synchronous. */
typedef struct hpn_bamsort_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t store_bytes;    /* bytes the record store holds after this call */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_bamsort_info;
typedef struct hpn_bamsort_result {
    uint64_t n_records, payload_bytes, fresh_mem;
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, sort_bits; /* sort_bits: the key bits [0, sort_bits) the radix sort ran over */
} hpn_bamsort_result;
int hpn_bam_sort_begin(hpn_ctx *ctx);
int hpn_bam_sort_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, hpn_bamsort_info *info);
int hpn_bam_sort_finish(hpn_ctx *ctx, hpn_bamsort_result *res);
int hpn_bam_sort_order(hpn_ctx *ctx, uint32_t *order, uint64_t n);
int hpn_bam_sort_sizes(hpn_ctx *ctx, uint32_t *sizes, uint64_t n);
int hpn_bam_sort_emit(hpn_ctx *ctx, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info);
int hpn_bam_sort_blocks(hpn_ctx *ctx, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n);
int hpn_bam_sort_payload_dev(hpn_ctx *ctx, const uint8_t **d_payload, uint64_t *n_bytes);
int hpn_bam_sort_stored_dev(hpn_ctx *ctx, const uint8_t **d_image, uint64_t *n_bytes);

/* ---- samtools rmdup: PCR duplicates of a coordinate-sorted BAM removed (pairs) -------------------
 * bam_rmdup.c (samtools-0.1.19), bam_rmdup_core: among the heads (paired, both mates mapped to one target, isize > 0) of one
 * (refID, pos, library, isize) the first one with the largest sum of qualities stays and leaves from the place of the group's
 * first record, behind everything of its (refID, pos) that is written at once; every other head's name goes into a set, and a
 * tail (isize <= 0) whose name is in the set is dropped.  The survivors are cut into BGZF blocks by bam_write1's rule (see
 * hpn_bam_split_*).  (docs/kernels/bam_rmdup.md)
 *   hpn_bam_rmdup_begin(n_ref, n_ids, ids, lib_of_id, n_libs)
 *              the header's @RG table: ID ids[k] (a C string) belongs to library lib_of_id[k] in [1, n_libs); library 0 is the
 *              one of records without an RG tag, with an ID the table lacks or whose @RG has no LB (the reference's "\t").
 *              Libraries are the caller's numbering of the distinct LB strings.
 *   per batch: hpn_bam_raw_index_dev(...), then hpn_bam_rmdup_add_raw_dev(d_raw, &info): the batch's records are classified and
 *              copied into the session's record store (d_raw may be reused afterwards); d_raw NULL: no records.  A batch may end
 *              anywhere: runs, groups and name events are made by _finish from what all batches left.
 *   hpn_bam_rmdup_finish(&res)            decides; res.n_out records survive, res.payload_bytes their bytes
 *   hpn_bam_rmdup_counts(libs, targets)   libs[l] (n_libs entries): heads checked and removed of library l and its first head's
 *                                         ordinal (-1: none; the order of first heads is the reference's insertion order, which
 *                                         decides the order of its summary lines); targets[t] (n_ref + 1 entries): whether
 *                                         target t has records and the names left in the set when it ends ("N unmatched
 *                                         pairs"); targets[n_ref].has_records: unplaced records follow the placed ones
 *   hpn_bam_rmdup_order(order, n)         order[j]: the input ordinal of the j-th record of the output (n = res.n_out)
 *   hpn_bam_rmdup_emit / _blocks / _payload_dev / _stored_dev    as hpn_bam_sort_emit and its three readers
 * Domain: (unsigned refID, pos) never goes backwards, pos >= 0 on every placed record, refID -1 only behind every placed record
 * and not on the first, every refID inside the header, fewer than 2^31 records; for heads and tails a name that ends with its
 * only NUL; for heads an RG tag of type Z and aux fields of the format's types that end inside the record; no name inserted into
 * the set twice.  The first record outside it is reported -- bad_record (ordinal, -1: none), bad_tid, bad_pos, reason
 * (HPN_RMDUP_*) -- and nothing is decided: the caller follows the reference on the host (csrc/host/bam_rmdup_host.hpp).
 * Synchronous. */
#define HPN_RMDUP_TID_BACK 1        /* a refID below the one before (unsigned), or a placed record behind an unplaced one */
#define HPN_RMDUP_POS_BACK 2        /* a pos below the one before on the same target */
#define HPN_RMDUP_RECORDS 3         /* the 2^31-th record */
#define HPN_RMDUP_RG_TYPE 4         /* a head's RG tag is not of type Z */
#define HPN_RMDUP_AUX 5             /* a head's aux fields: a type outside AcCsSiIfZHB, or a field that ends behind the record */
#define HPN_RMDUP_NAME 6            /* a head's or tail's name: l_read_name 0, a NUL inside it or none at its end */
#define HPN_RMDUP_INCONSISTENT 7    /* "inconsistent BAM file for pair": a name inserted into the set while it is in it */
#define HPN_RMDUP_COLLISION 8       /* two different names with one 64-bit hash */
#define HPN_RMDUP_FIRST_UNPLACED 9  /* the file begins with refID -1 */
#define HPN_RMDUP_TID_BEYOND 10     /* a refID the header does not have */
#define HPN_RMDUP_POS_NEG 11        /* pos below 0 on a placed record */
#define HPN_RMDUP_FIELDS 12         /* a head's fixed fields lead outside the record */
typedef struct hpn_rmdup_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t store_bytes;    /* bytes the record store holds after this call */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_rmdup_info;
typedef struct hpn_rmdup_result {
    uint64_t n_records, n_out, payload_bytes, n_heads;
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, n_libs, n_ref, reserved;
} hpn_rmdup_result;
typedef struct hpn_rmdup_lib {
    uint64_t checked, removed;
    int64_t first;
} hpn_rmdup_lib;
typedef struct hpn_rmdup_target {
    uint64_t unmatched;
    uint32_t has_records, reserved;
} hpn_rmdup_target;
int hpn_bam_rmdup_begin(hpn_ctx *ctx, int32_t n_ref, uint32_t n_ids, const char *const *ids, const uint32_t *lib_of_id, uint32_t n_libs);
int hpn_bam_rmdup_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, hpn_rmdup_info *info);
int hpn_bam_rmdup_finish(hpn_ctx *ctx, hpn_rmdup_result *res);
int hpn_bam_rmdup_counts(hpn_ctx *ctx, hpn_rmdup_lib *libs /* [n_libs] */, hpn_rmdup_target *targets /* [n_ref + 1] */);
int hpn_bam_rmdup_order(hpn_ctx *ctx, uint32_t *order, uint64_t n);
int hpn_bam_rmdup_emit(hpn_ctx *ctx, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info);
int hpn_bam_rmdup_blocks(hpn_ctx *ctx, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n);
int hpn_bam_rmdup_payload_dev(hpn_ctx *ctx, const uint8_t **d_payload, uint64_t *n_bytes);
int hpn_bam_rmdup_stored_dev(hpn_ctx *ctx, const uint8_t **d_image, uint64_t *n_bytes);

/* ---- samtools merge: several BAMs merged into one ------------------------------------------------
 * bam_sort.c (samtools-0.1.19), bam_merge_core2, for the order by coordinate: a heap over one record per input file, ordered by
 * (uint64_t)refID << 32 | (uint32_t)(pos + 1) << 1 | strand (strand: flag 0x10; the low word is cut to 32 bits, so every pos has
 * its key), ties to the lower file number.  The reference never checks that its inputs are sorted; for any inputs what the heap
 * writes is the records, file after file in argument order, sorted stably by their EFFECTIVE key: the largest key of the
 * record's own file up to and including the record.  The session computes exactly that, and cuts the result into BGZF blocks by
 * bam_write1's rule (see hpn_bam_split_*).  (docs/kernels/bam_merge.md)
 *   hpn_bam_merge_begin()
 *   per input file, in argument order: hpn_bam_merge_next_file() -- it closes the file before it; a file of no records is legal --
 *   then per batch of that file: hpn_bam_raw_index_dev(...), then hpn_bam_merge_add_raw_dev(d_raw, &info): the batch's records
 *              are copied into the session's record store on the device (d_raw may be reused afterwards); d_raw NULL: no records
 *   hpn_bam_merge_finish(&res)            merges; res.n_files: the hpn_bam_merge_next_file calls, res.payload_bytes: the records'
 *                                         bytes, res.n_lifted: the records whose effective key is not their own -- 0 exactly
 *                                         when every file was sorted by the heap's key
 *   hpn_bam_merge_order(order, n)         order[j]: the session ordinal (files in argument order, records in file order) of the
 *                                         j-th record of the output (n = res.n_records)
 *   hpn_bam_merge_emit / _blocks / _payload_dev / _stored_dev    as hpn_bam_sort_emit and its three readers
 * Domain: no record with the key 2^64 - 1 (refID -1, reverse strand, pos -2 or 2^31 - 2: the heap's HEAP_EMPTY, where the
 * reference ends its output) and fewer than 2^31 records.  The first record outside it is reported -- bad_record (session
 * ordinal, -1: none), bad_tid, bad_pos, reason (1 the HEAP_EMPTY key, 2 the 2^31-th record) -- and nothing is merged: the caller
 * merges on the host (csrc/host/bam_merge_host.hpp).  A call out of this order returns HPN_E_STATE.  Synchronous. */
typedef struct hpn_bammerge_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t store_bytes;    /* bytes the record store holds after this call */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_bammerge_info;
typedef struct hpn_bammerge_result {
    uint64_t n_records, n_files, payload_bytes, n_lifted;
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, sort_bits; /* sort_bits: the key bits [0, sort_bits) the radix sort ran over */
} hpn_bammerge_result;
int hpn_bam_merge_begin(hpn_ctx *ctx);
int hpn_bam_merge_next_file(hpn_ctx *ctx);
int hpn_bam_merge_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, hpn_bammerge_info *info);
int hpn_bam_merge_finish(hpn_ctx *ctx, hpn_bammerge_result *res);
int hpn_bam_merge_order(hpn_ctx *ctx, uint32_t *order, uint64_t n);
int hpn_bam_merge_emit(hpn_ctx *ctx, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info);
int hpn_bam_merge_blocks(hpn_ctx *ctx, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n);
int hpn_bam_merge_payload_dev(hpn_ctx *ctx, const uint8_t **d_payload, uint64_t *n_bytes);
int hpn_bam_merge_stored_dev(hpn_ctx *ctx, const uint8_t **d_image, uint64_t *n_bytes);

/* ---- samtools fixmate: mate fields of a name-grouped BAM filled in -------------------------------
 * bam_mate.c (samtools-0.1.19), bam_mating_core: over the records in file order with one pending record.  A record with
 * refID < 0 is written at once (dropped with remove_reads); otherwise flag 0x4 is set where bam_calend lies beyond the target's
 * length, and a record with flag 0x100 is written at once (dropped with remove_reads).  Every other record is LIVE: two live
 * records in a row with the same name are a pair -- both get the other's refID and pos as mate fields, the insert size from the
 * 5' ends (0 unless both lie on one target and neither has 0x4 or 0x8), 0x20 from the other's 0x10, 0x8 without 0x2 where the
 * other has 0x4, and on one target the record with the smaller pos gets a CT:Z field appended (bam_template_cigar) --, a live
 * record followed by another name is a singleton (mate fields -1, -1, 0; with 0x1: 0x8 set, 0x20 and 0x2 cleared), and the
 * pending record at the end of the file is written as it is.  The output's order is not the input's: a skipped record is written
 * in front of a pending one that came earlier.  (docs/kernels/bam_fixmate.md)
 *   hpn_bam_fixmate_begin(remove_reads, n_targets, target_len)      the header's l_ref values (copied)
 *   per batch: hpn_bam_raw_index_dev(...), then hpn_bam_fixmate_add_raw_dev(d_raw, &info): the batch's records are copied into
 *              the session's record store on the device (d_raw may be reused afterwards); d_raw NULL: no records.  A pair may lie
 *              in two batches.
 *   hpn_bam_fixmate_finish(&res)          decides; res.n_out records leave, res.payload_bytes their bytes (bytes_added of them CT
 *                                         fields, n_tags of them)
 *   hpn_bam_fixmate_order(order, n)       order[j]: the session ordinal of the j-th record of the output (n = res.n_out)
 *   hpn_bam_fixmate_emit / _blocks / _payload_dev / _stored_dev    as hpn_bam_sort_emit and its three readers; the records of a
 *                                         slice are rewritten (five core fields, the CT field) before they are cut and summed
 * Domain: CIGAR ops 0..8 (reason 1), live records' names with their first NUL as their last byte (2), refID < n_targets (3), a
 * name and CIGAR inside the record (4), fewer than 2^31 records (5).  The first record outside it is reported -- bad_record
 * (session ordinal, -1: none), bad_tid, bad_pos, reason -- and nothing is fixed: the caller works on the host
 * (csrc/host/bam_fixmate_host.hpp).  A call out of this order returns HPN_E_STATE.  Synchronous. */
typedef struct hpn_fixmate_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t store_bytes;    /* bytes the record store holds after this call */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_fixmate_info;
typedef struct hpn_fixmate_result {
    uint64_t n_records, n_out;                  /* records in, records out */
    uint64_t n_pairs, n_singletons, n_tags;     /* pairs, singletons (the pending record at the end is none), CT fields */
    uint64_t bytes_added, payload_bytes;
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_fixmate_result;
int hpn_bam_fixmate_begin(hpn_ctx *ctx, int remove_reads, int32_t n_targets, const uint32_t *target_len);
int hpn_bam_fixmate_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, hpn_fixmate_info *info);
int hpn_bam_fixmate_finish(hpn_ctx *ctx, hpn_fixmate_result *res);
int hpn_bam_fixmate_order(hpn_ctx *ctx, uint32_t *order, uint64_t n);
int hpn_bam_fixmate_emit(hpn_ctx *ctx, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info);
int hpn_bam_fixmate_blocks(hpn_ctx *ctx, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n);
int hpn_bam_fixmate_payload_dev(hpn_ctx *ctx, const uint8_t **d_payload, uint64_t *n_bytes);
int hpn_bam_fixmate_stored_dev(hpn_ctx *ctx, const uint8_t **d_image, uint64_t *n_bytes);

/* ---- samtools view: a BAM's records filtered, as BAM, as SAM text or counted ----------------------
 * sam_view.c (samtools-0.1.19), process_aln: a record is dropped where the CIGAR's query length (ops whose type has bit 1, and H)
 * is below min_qlen (> 0), mapq < min_mapq, (flag & flag_on) != flag_on, flag & flag_off, or, with subsample, where
 * ((X31(name) + seed) & 0xffffff) >= threshold -- X31 = __ac_X31_hash_string over signed chars, threshold the 24-bit integer the
 * caller derives from the fraction: ceil(frac * 2^24), at most 2^24.  qual_scale > 1 turns every quality byte q into
 * min(q * scale, 93), in BAM and in text output alike.  Text is bam_format1_core's line (bam.c) and a newline, the flag decimal,
 * 0x%x or by bam_flag2char_table.  The order is the input's.  (docs/kernels/bam_view.md)
 *   hpn_bam_view_begin(&opts)             the rules, what the session emits and, for text, the targets' names (copied)
 *   per batch: hpn_bam_raw_index_dev(...), then hpn_bam_view_add_raw_dev(d_raw, &info): the batch's records are classified and
 *              copied into the session's record store on the device; d_raw NULL: no records
 *   hpn_bam_view_finish(&res)             res.n_out records are kept: the count.  payload_bytes their bytes as BAM (HPN_VIEW_BAM),
 *                                         text_bytes their lines' bytes (HPN_VIEW_TEXT)
 *   hpn_bam_view_order(order, n)          order[j]: the session ordinal of the j-th kept record (n = res.n_out)
 *   HPN_VIEW_BAM:  hpn_bam_view_emit / _blocks / _payload_dev / _stored_dev    as hpn_bam_sort_emit and its three readers
 *   HPN_VIEW_TEXT: hpn_bam_view_text_emit(first_record, max_records, &info) formats output records [first, first + n) -- the
 *                  next ones: first is where the call before ended -- into a device buffer, hpn_bam_view_text_dev(&d_text,
 *                  &n_bytes) names it until the next call
 *   The read-group rule (-r, -R, -l): one lane walks the aux fields to RG as bam_aux_get does and compares the value with the
 *   ID table of hpn_view_opts; the caller derives lib_ids from the header's @RG lines (ID -> LB).
 *   A BAM call on a text or count session, and a text call on any other, returns HPN_E_STATE.
 * Domain, where the record's inside is read (text: all of it; -m, -s, qual_scale and the read-group rule: what they read): no f, d or B:f aux field
 * (reason 1), no A field of value 0 (2), a name whose first NUL is its last byte (3), known aux types and B counts >= 0 (4),
 * name, CIGAR, sequence, qualities and every aux field inside the record (5), pos and mpos below 2^31 - 1 (6), fewer than 2^31
 * records (7), refID and mate refID < n_targets (8), CIGAR ops 0..9 (9).  The first record outside it is reported -- bad_record
 * (session ordinal, -1: none), bad_tid, bad_pos, reason -- and nothing is emitted: the caller works on the host
 * (csrc/host/bam_view_host.hpp).  A call out of this order returns HPN_E_STATE.  Synchronous. */
#define HPN_VIEW_BAM 0
#define HPN_VIEW_TEXT 1
#define HPN_VIEW_COUNT 2
typedef struct hpn_view_opts {
    uint32_t flag_on, flag_off, min_mapq;
    int32_t min_qlen, qual_scale;
    uint32_t subsample, seed, threshold;   /* subsample != 0: on */
    uint32_t emit;                         /* HPN_VIEW_BAM, _TEXT or _COUNT */
    uint32_t flag_style;                   /* text: 0 decimal, 1 hexadecimal (-x), 2 letters (-X) */
    int32_t n_targets;                     /* text: the header's targets */
    uint32_t reserved;
    const char *target_names;              /* text: their names behind one another, without NULs ... */
    const uint32_t *target_name_off;       /* ... name t is bytes [off[t], off[t + 1]); n_targets + 1 entries */
    /* the read-group rule, C strings (copied): a record WITH an RG field is decided by rg_id (-r) if given, else by the set
     * rg_ids (-R) if has_rg_ids; a record the two leave undecided -- it has no RG field, or neither is given -- is kept only if
     * its RG value is one of lib_ids, the IDs whose LB is the library (-l), if has_library; without the three nothing is read */
    const char *rg_id;                     /* NULL: no -r */
    const char *const *rg_ids;
    const char *const *lib_ids;
    uint32_t n_rg_ids, n_lib_ids;
    uint32_t has_rg_ids, has_library;      /* an empty set still rules: it keeps nothing it decides */
    uint64_t reserved2[4];                 /* 0 */
} hpn_view_opts;
typedef struct hpn_view_info {
    uint64_t n_records;      /* records of this batch */
    uint64_t store_bytes;    /* bytes the record store holds after this call */
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_view_info;
typedef struct hpn_view_result {
    uint64_t n_records, n_out;                  /* records in, records kept */
    uint64_t payload_bytes, text_bytes;
    int64_t bad_record;
    int32_t bad_tid, bad_pos;
    uint32_t reason, reserved;
} hpn_view_result;
typedef struct hpn_view_text_info {
    uint64_t n_records, n_bytes;                /* the slice's lines and their bytes */
} hpn_view_text_info;
int hpn_bam_view_begin(hpn_ctx *ctx, const hpn_view_opts *opts);
int hpn_bam_view_add_raw_dev(hpn_ctx *ctx, const uint8_t *d_raw, hpn_view_info *info);
int hpn_bam_view_finish(hpn_ctx *ctx, hpn_view_result *res);
int hpn_bam_view_order(hpn_ctx *ctx, uint32_t *order, uint64_t n);
int hpn_bam_view_emit(hpn_ctx *ctx, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info);
int hpn_bam_view_blocks(hpn_ctx *ctx, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n);
int hpn_bam_view_payload_dev(hpn_ctx *ctx, const uint8_t **d_payload, uint64_t *n_bytes);
int hpn_bam_view_stored_dev(hpn_ctx *ctx, const uint8_t **d_image, uint64_t *n_bytes);
int hpn_bam_view_text_emit(hpn_ctx *ctx, uint64_t first_record, uint64_t max_records, hpn_view_text_info *info);
int hpn_bam_view_text_dev(hpn_ctx *ctx, const uint8_t **d_text, uint64_t *n_bytes);

/* ---- multi-GPU reduction of count vectors -----------------------------------
 * One RCCL communicator per context; `unique_id` is the 128-byte ncclUniqueId
 * produced by hpn_comm_unique_id on rank 0 and handed to every rank by the host
 * program (file, pipe, torch.distributed ...).  hpn_allreduce_u64 sums a device
 * vector in place over xGMI. */
#define HPN_UNIQUE_ID_BYTES 128
int hpn_comm_unique_id(uint8_t id[HPN_UNIQUE_ID_BYTES]);
int hpn_comm_init(hpn_ctx *ctx, int rank, int n_ranks, const uint8_t id[HPN_UNIQUE_ID_BYTES]);
int hpn_comm_destroy(hpn_ctx *ctx);
int hpn_allreduce_u64(hpn_ctx *ctx, uint64_t *d_vec, size_t n);
/* The same for ONE process that owns several contexts (the C tools sharding one input over the node's
 * GPUs): hpn_comm_init_all builds one communicator per context (ncclCommInitAll; the contexts must sit
 * on n distinct devices, else HPN_E_ARG and nothing is made -- callers then add the vectors on the
 * host), hpn_allreduce_u64_all sums d_vecs[i] (on ctxs[i]'s device) in place into every one of them in
 * one RCCL group, each on its context's stream; the call returns when all have finished.  This is where
 * reduceStats' element-wise sum goes (fastq_count_kthread.c:180-210).  A failure before anything was
 * enqueued (HPN_E_RCCL / HPN_E_HIP) leaves the vectors as they were: the caller may add them on the
 * host; HPN_E_PARTIAL does not.  No path returns with the RCCL group open.  hpn_comm_library: the path of
 * the RCCL library the binding resolved to ("" before the first use / when none could be loaded). */
int hpn_comm_init_all(hpn_ctx **ctxs, int n);
int hpn_allreduce_u64_all(hpn_ctx **ctxs, uint64_t **d_vecs, int n, size_t n_words);
const char *hpn_comm_library(void);
/* Ranks of the context's communicator as RCCL itself reports them (ncclCommCount): what bench.py
 * prints beside n_gpus, so that a job that believes it has N ranks and a communicator of one cannot
 * pass for an N-GPU run.  HPN_E_STATE without a communicator. */
int hpn_comm_count(hpn_ctx *ctx, int *n_ranks);

/* ---- synthetic inputs, generated in HBM -----------------------------------
 * Counter-based: byte k of record r depends only on (seed, r, k), so any shard
 * can be produced independently and checked on the CPU.  Quality bytes uniform
 * in 35..74, bases A/C/G/T 24.75 % each + N 1 %.  Fixed read length `len`;
 * d_off gets (first_record-relative) offsets i*len as uint64. */
int hpn_synth_fastq_dev(hpn_ctx *ctx, uint64_t seed, uint64_t first_record, uint64_t n_records,
                        uint32_t len, uint8_t *d_qual, uint8_t *d_base_or_null, uint64_t *d_off);

#ifdef __cplusplus
}
#endif
#endif /* HPNGS_H */
