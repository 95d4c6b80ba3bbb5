// hpn_usort.hip -- C ABI of duplicate removal with an abundance order (gzfastq_uniq_sort.c): hpn_fastq_usort_begin / _add /
// _finish / _write.  Kernels: kernels/fastq_usort.hip; the store (hpn_store.hpp) and the grouping stage (hpn_uniq_group.hpp) are
// those of hpn_fastq_uniq_*, run over a session of its own.
//
// The reference sizes its table before it reads a record: count_read (gzfastq_uniq_sort.c:174-185) counts the gzgets that open
// a group of four lines of mate 1 -- e = ceil(lines / 4) -- and the table gets S = (size_t)(1.34 * e) slots.  hashtbl_insert
// would resize at count >= 0.75 * S, but U - 1 <= e - 1 < 0.75 * (1.34 e - 1) for every e >= 1: the table keeps its size and a
// chain holds its keys newest first.  The session counts mate 0's lines itself, so a caller cannot pass another table size.
#include "hpn_uniq_group.hpp"

namespace hpn {
// kernels/fastq_usort.hip
enum { kUsMaxCount = 7, kUsFirstSeq = 8, kUsSeqLen = 9, kUsShortKey = 10, kUsLongKey = 11 };
hipError_t launch_usort_seqlen(const void *d0, uint32_t n, uint32_t *d_info, hipStream_t st);
hipError_t launch_usort_djb64(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint32_t *d_first,
                              uint32_t n_groups, uint64_t *d_hash, hipStream_t st);
hipError_t launch_usort_bucket(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint32_t *d_first,
                               const uint32_t *d_rank, const uint32_t *d_count, const uint64_t *d_hash, uint32_t n_groups,
                               uint64_t table_size, uint64_t *d_key, uint32_t *d_val, uint32_t *d_info, hipStream_t st);
hipError_t launch_usort_count_key(const uint32_t *d_val, const uint32_t *d_count, uint32_t n_groups, uint64_t *d_key, hipStream_t st);
hipError_t launch_usort_sizes(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, int mate,
                              const uint32_t *d_list, const uint32_t *d_first, const uint32_t *d_count, uint32_t n_groups, uint32_t seq_len,
                              uint64_t *d_size, hipStream_t st);
hipError_t launch_usort_write(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, int mate,
                              const uint32_t *d_list, const uint32_t *d_first, const uint32_t *d_count, const uint64_t *d_off,
                              uint32_t n_groups, uint32_t seq_len, uint8_t *d_out, int n_cu, hipStream_t st);
}  // namespace hpn

using namespace hpn;

struct hpn_usort_work {   // what a new session must not inherit
    Scratch djb64, list, size64;
    uint64_t lone_line = 0;   // mate 0 ends with one line without '\n' behind its last record: count_read counts it
    uint32_t seq_len = 0;
};

struct hpn_usort_state : FamilyState, hpn_usort_work {
    static constexpr int kSlot = kStUsort;
    hpn_uniq_state g;   // the store, the grouping stage's arrays, the output text
};

namespace {

void drop_session(hpn_usort_state *q)
{
    uniq_drop_session(&q->g);
    static_cast<hpn_usort_work &>(*q) = hpn_usort_work();
}

// the whole text of one mate's output on the device (u->out, u->out_total bytes)
int build_output(hpn_ctx *c, hpn_usort_state *q, int mate)
{
    hpn_uniq_state *u = &q->g;
    int rc;
    const uint32_t U = u->U;
    const int paired = u->paired;
    if ((rc = need(c, q->size64, (size_t)U * 8)) != HPN_OK || (rc = need(c, u->off, ((size_t)U + 1) * 8)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(U) * 8)) != HPN_OK)
        return rc;
    const uint8_t *t0 = (const uint8_t *)u->s.m[0].store.p + kStorePad, *t1 = paired ? (const uint8_t *)u->s.m[1].store.p + kStorePad : nullptr;
    const void *d0 = u->s.m[0].desc.p, *d1 = paired ? u->s.m[1].desc.p : nullptr;
    const uint32_t *list = (const uint32_t *)q->list.p, *first = (const uint32_t *)u->first.p, *count = (const uint32_t *)u->count.p;
    HPN_HIP(c, launch_usort_sizes(t0, d0, t1, d1, paired, mate, list, first, count, U, q->seq_len, (uint64_t *)q->size64.p, c->stream));
    HPN_HIP(c, uniq_scan64w((const uint64_t *)q->size64.p, (uint64_t *)u->off.p, U, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(),
                            c->stream));
    uint64_t total = 0;
    HPN_HIP(c, hipMemcpyAsync(&total, (const uint64_t *)u->off.p + U, 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    u->cached_mate = -1;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_usort_write(t0, d0, t1, d1, paired, mate, list, first, count, (const uint64_t *)u->off.p, U, q->seq_len,
                                  (uint8_t *)u->out.p, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    u->out_total = total;
    u->cached_mate = mate;
    return HPN_OK;
}

int bits_of(uint64_t v)
{
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

}  // namespace

extern "C" {

int hpn_fastq_usort_begin(hpn_ctx *c, int paired, uint64_t max_bytes, uint32_t hash_bits)
{
    if (!c) return HPN_E_ARG;
    if (hash_bits > 63) return fail(c, HPN_E_ARG, "hash_bits %u (0 = all 64, or 1 .. 63)", hash_bits);
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_usort_state *q = state_make<hpn_usort_state>(c);
    drop_session(q);
    return uniq_begin(c, &q->g, paired, max_bytes, hash_bits);
}

int hpn_fastq_usort_add(hpn_ctx *c, int mate, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_usort_state *q = state<hpn_usort_state>(c);
    const uint64_t span = q && mate == 0 ? q->g.s.m[0].len - q->g.s.m[0].pos + nbytes : 0;   // (what the call frames, when it gets that far)
    const int rc = session_add(c, q ? &q->g.s : nullptr, "hpn_fastq_usort", mate, kUniqDescBytes, frame_by<launch_uniqq_keys>, nullptr, 4u, text, nbytes, last, false, info);
    // the line index of the stream's last stretch tells whether one open line follows the last record (k_uniq_keys takes it as
    // no record; count_read's gzgets returns it)
    if (rc == HPN_OK && q->g.s.open && last && mate == 0 && span)
        q->lone_line = (c->h_tstate[kTsLines] & 3u) == 1u && c->h_tstate[kTsUnterminated] ? 1 : 0;
    return rc;
}

int hpn_fastq_usort_finish(hpn_ctx *c, hpn_usort_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_usort_state *q = state<hpn_usort_state>(c);
    hpn_uniq_state *u = q ? &q->g : nullptr;
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_fastq_usort", kUniqDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    res->unmatched = -1;
    const int paired = u->paired;
    const uint8_t *t0 = u->s.text(0), *t1 = paired ? u->s.text(1) : nullptr;
    const void *d0 = u->s.m[0].desc.p, *d1 = paired ? u->s.m[1].desc.p : nullptr;
    HPN_HIP(c, hipMemsetAsync(uniq_kinfo(u) + kUsFirstSeq, 0xff, sizeof(uint32_t), c->stream));
    const uint64_t e = u->s.m[0].n + q->lone_line;
    const uint64_t S = (uint64_t)(1.34 * (double)e);   // HSIZE tblsiz=1.34*elecnt (:117)
    res->table_reads = e, res->hash_size = S;
    uint32_t N = (uint32_t)u->s.m[0].n;
    if ((rc = uniq_match_mates(c, u, &N, &res->unmatched, res->unmatched_name)) != HPN_OK) return rc;
    u->N = N;
    res->n_records = N;
    if (N && e < 10) {   // total_reads_count % (elecnt / 10) behind the first record (:161)
        u->s.open = false;
        res->no_answer = HPN_USORT_FEW_READS;
        return fail(c, HPN_E_DOMAIN, "%llu reads counted: the reference divides by %llu / 10 = 0 behind its first record", (unsigned long long)e,
                    (unsigned long long)e);
    }
    uint64_t walk_size = 0;
    if ((rc = uniq_group(c, u, false, &walk_size, &res->hash_clashes)) != HPN_OK) return rc;
    const uint32_t U = u->U;
    res->n_unique = U;
    if ((rc = need(c, q->djb64, (size_t)U * 8)) != HPN_OK || (rc = need(c, q->list, (size_t)U * 4)) != HPN_OK) return rc;
    uint64_t *key = (uint64_t *)u->key.p;
    uint32_t *val = (uint32_t *)u->val.p;
    const uint32_t *first = (const uint32_t *)u->first.p, *count = (const uint32_t *)u->count.p;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTally], c->stream));
    // (strLen is set in front of the pair test, :129: the mate-0 record at which the pairs stop still counts)
    HPN_HIP(c, launch_usort_seqlen(d0, res->unmatched >= 0 ? N + 1u : N, uniq_kinfo(u), c->stream));
    HPN_HIP(c, launch_usort_djb64(t0, d0, t1, d1, paired, first, U, (uint64_t *)q->djb64.p, c->stream));
    HPN_HIP(c, launch_usort_bucket(t0, d0, t1, d1, paired, first, (const uint32_t *)u->rank.p, count, (const uint64_t *)q->djb64.p, U, S, key, val,
                                   uniq_kinfo(u), c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    res->max_count = u->s.info.h[kUiBase + kUsMaxCount];
    res->seq_len = q->seq_len = u->s.info.h[kUiBase + kUsSeqLen];
    if (u->s.info.h[kUiBase + kUsLongKey] || u->s.info.h[kUiBase + kUsShortKey]) {
        u->s.open = false;
        res->no_answer = u->s.info.h[kUiBase + kUsLongKey] ? HPN_USORT_LONG_KEY : HPN_USORT_SHORT_KEY;
        return u->s.info.h[kUiBase + kUsLongKey] ? fail(c, HPN_E_DOMAIN, "a pair's joined sequences have more than 1023 bytes: the reference's key buffer holds 1024")
                                     : fail(c, HPN_E_DOMAIN, "a pair's joined sequences have fewer than the %u bytes of the first read: the reference prints from behind the key", q->seq_len);
    }
    // the walk: slots ascending, every chain newest first; then count descending over the digits that can differ
    if ((rc = uniq_sort(c, u, key, val, U, 0, S > 1 ? bits_of(S - 1) : 0)) != HPN_OK) return rc;
    HPN_HIP(c, launch_usort_count_key(val, count, U, key, c->stream));
    if ((rc = uniq_sort(c, u, key, val, U, 0, bits_of(res->max_count))) != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(q->list.p, val, (size_t)U * 4, hipMemcpyDeviceToDevice, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTally], c->stream));
    u->s.finished = true;
    for (int k = paired; k >= 0; --k) {   // (mate 0 last: its text stays built for the first hpn_fastq_usort_write)
        if ((rc = build_output(c, q, k)) != HPN_OK) return rc;
        res->out_bytes[k] = u->out_total;
    }
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

int hpn_fastq_usort_write(hpn_ctx *c, int mate, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_usort_state *q = state<hpn_usort_state>(c);
    hpn_uniq_state *u = q ? &q->g : nullptr;
    int rc;
    if ((rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_fastq_usort", written)) != HPN_OK) return rc;
    if (mate < 0 || mate > u->paired) return fail(c, HPN_E_ARG, "mate %d of a %s session", mate, u->paired ? "paired" : "single-end");
    if (u->cached_mate != mate && (rc = build_output(c, q, mate)) != HPN_OK) return rc;
    return session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

}  // extern "C"
