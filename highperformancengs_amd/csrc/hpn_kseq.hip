// hpn_kseq.hip -- C ABI of map_kseq.cpp / kbtree_kseq.c: hpn_kseq_begin / _add / _finish / _write.
// Kernels: kernels/kseq_frame.hip (the framing, the heads of the runs, the writer), the refinement sort of kernels/fastq_sort.hip
// in its third key mode (hpn_sort.hip: sort_state_order), the scans of kernels/fastq_uniq.hip, the line index of
// kernels/fastq_text.hip.  The stream lies in the session's store (hpn_store.hpp) and is framed chunk by chunk, an unfinished
// record staying unframed; what is framed is copied into a second, NORMALISED store -- "name comment\nsequence\n[quality]" per
// record, the sequence's lines joined -- which the descriptors (SortDesc) point into and everything behind the framing reads.
#include "hpn_store.hpp"
#include "kernels/sort_desc.hpp"

namespace hpn {
struct KseqLines {   // kernels/kseq_frame.hip
    uint32_t *hdr, *t, *ne, *hid, *P, *NE, *hline, *x;
};
constexpr size_t kKseqRecBytes = 32;   // sizeof(KseqRec)
// kernels/kseq_frame.hip
hipError_t launch_kseq_fq_recs(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint32_t n_lines,
                               void *d_rec, uint32_t *d_rsize, uint32_t *d_state, hipStream_t st);
hipError_t launch_kseq_fa_lines(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t n_lines, const KseqLines &a,
                                uint32_t *d_state, hipStream_t st);
hipError_t launch_kseq_fa_recs(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint32_t n_lines,
                               const KseqLines &a, void *d_rec, uint32_t *d_rsize, uint32_t *d_state, hipStream_t st);
hipError_t launch_kseq_fa_copy(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, int last, uint32_t n_lines, const KseqLines &a,
                               const void *d_rec, const uint64_t *d_roff, uint8_t *d_dst, int n_cu, hipStream_t st);
hipError_t launch_kseq_put(const uint8_t *d_slot, const void *d_rec, const uint64_t *d_roff, const uint32_t *d_state, uint32_t max_records,
                           int fastq, uint8_t *d_norm, uint64_t origin, void *d_desc, int n_cu, hipStream_t st);
hipError_t launch_kseq_heads(const uint8_t *d_text, const void *d_desc, const uint32_t *d_order, uint32_t n, uint32_t *d_head,
                             uint32_t *d_info, hipStream_t st);
hipError_t launch_kseq_pick(const void *d_desc, const uint32_t *d_order, const uint32_t *d_head, const uint32_t *d_at, uint32_t n, int fastq,
                            uint32_t *d_pick, uint32_t *d_size, hipStream_t st);
hipError_t launch_kseq_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_pick, const uint64_t *d_off, uint32_t n, int fastq,
                             uint8_t *d_out, int n_cu, hipStream_t st);
// hpn_sort.hip
hpn_sort_state *sort_state_new(hpn_ctx *c);
void sort_state_free(hpn_sort_state *u);
void sort_state_drop(hpn_sort_state *u);   // its arrays; the state stays
int sort_state_order(hpn_ctx *c, hpn_sort_state *u, const uint8_t *text, const void *desc, uint32_t n, uint32_t *rounds, uint64_t *refined,
                     const uint32_t **d_order);
}  // namespace hpn

using namespace hpn;

namespace {
enum { kKiOther = kInfoOwn };   // the family's word of the info block: the first record whose length is not the first record's
}

struct hpn_kseq_state {
    StoreSession s;        // m[0]: the stream as it came; its descriptors point into `norm`
    Scratch norm;          // kStorePad, the normalised records, kStorePad
    uint64_t norm_len = 0;
    uint32_t shape = HPN_KSEQ_NONE;
    hpn_sort_state *sorter = nullptr;
    Scratch l_hdr, l_t, l_ne, l_hid, l_P, l_NE, l_hline, l_x, rec, rsize, roff, status;   // the framing's arrays, per chunk
    Scratch head, at, pick, size, off, out;                                               // _finish
    uint64_t out_total = 0;
    hpn_ctx *ctx = nullptr;   // the framing's way back to the context (store_add hands it the state as `user`)
    int frame_rc = HPN_OK;    // what an allocation inside the framing returned, and the message it left
    char frame_err[sizeof(hpn_ctx::err)] = {0};
};

namespace {

void drop_session(hpn_kseq_state *u)
{
    session_drop(u->s);
    Scratch *ss[] = {&u->norm, &u->l_hdr, &u->l_t, &u->l_ne, &u->l_hid, &u->l_P, &u->l_NE, &u->l_hline, &u->l_x, &u->rec, &u->rsize,
                     &u->roff, &u->status, &u->head, &u->at, &u->pick, &u->size, &u->off, &u->out};
    for (Scratch *s : ss) release_scratch(*s);
    u->norm_len = 0, u->shape = HPN_KSEQ_NONE, u->out_total = 0;
    if (u->sorter) sort_state_drop(u->sorter);
}

// an allocation (or a scan) inside the framing failed: the status and the message are kept for _add, which closes the session
hipError_t frame_failed(hpn_ctx *c, hpn_kseq_state *u, int rc)
{
    u->frame_rc = rc;
    memcpy(u->frame_err, c->err, sizeof u->frame_err);
    return hipErrorOutOfMemory;
}

// The chunk's records into the normalised store and their descriptors (store_frame_fn).  max_records is the chunk's line count.
hipError_t kseq_frame(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin, void *d_desc,
                      uint32_t max_records, uint32_t *d_state, hipStream_t st, void *user)
{
    (void)origin;
    hpn_kseq_state *u = (hpn_kseq_state *)user;
    hpn_ctx *c = u->ctx;
    const uint32_t L = max_records;
    const bool fastq = u->shape == HPN_KSEQ_FASTQ;
    const uint32_t kmax = fastq ? L / 4u : (L + 1u) / 2u;
    int rc;
    hipError_t e;
#define KSEQ_NEED(s, bytes) \
    if ((rc = need(c, (s), (bytes))) != HPN_OK) return frame_failed(c, u, rc)
    KSEQ_NEED(u->rec, ((size_t)kmax + 1) * kKseqRecBytes);
    KSEQ_NEED(u->rsize, ((size_t)kmax + 1) * 4);
    KSEQ_NEED(u->roff, ((size_t)kmax + 2) * 8);
    KSEQ_NEED(u->status, uniq_scan_tiles((uint64_t)L + 1) * 8);
    KseqLines a = {};
    if (fastq) {
        if ((e = launch_kseq_fq_recs(d_slot, d_nl, begin, end, last, L, u->rec.p, (uint32_t *)u->rsize.p, d_state, st)) != hipSuccess) return e;
    } else {
        Scratch *per[] = {&u->l_hdr, &u->l_t, &u->l_ne, &u->l_hid, &u->l_P, &u->l_NE, &u->l_hline, &u->l_x};
        for (Scratch *s : per) KSEQ_NEED(*s, ((size_t)L + 2) * 4);
        a = KseqLines{(uint32_t *)u->l_hdr.p, (uint32_t *)u->l_t.p,  (uint32_t *)u->l_ne.p,    (uint32_t *)u->l_hid.p,
                      (uint32_t *)u->l_P.p,   (uint32_t *)u->l_NE.p, (uint32_t *)u->l_hline.p, (uint32_t *)u->l_x.p};
        u64 *status = (u64 *)u->status.p;
        if ((e = launch_kseq_fa_lines(d_slot, d_nl, begin, L, a, d_state, st)) != hipSuccess) return e;
        if ((e = uniq_scan32(a.hdr, a.hid, L, status, u->s.ticket(), u->s.err(), st)) != hipSuccess) return e;
        if ((e = uniq_scan32(a.t, a.P, L, status, u->s.ticket(), u->s.err(), st)) != hipSuccess) return e;
        if ((e = uniq_scan32(a.ne, a.NE, L, status, u->s.ticket(), u->s.err(), st)) != hipSuccess) return e;
        if ((e = launch_kseq_fa_recs(d_slot, d_nl, begin, end, last, L, a, u->rec.p, (uint32_t *)u->rsize.p, d_state, st)) != hipSuccess) return e;
    }
    if ((e = uniq_scan64((const uint32_t *)u->rsize.p, (uint64_t *)u->roff.p, kmax, (u64 *)u->status.p, u->s.ticket(), u->s.err(), st)) != hipSuccess)
        return e;
    // the chunk's bytes in the normalised store, and whether the chunk is regular at all: both on the host before the copies
    uint64_t total = 0;
    uint32_t flags = 0, scan_err = 0;
    if ((e = hipMemcpyAsync(&total, (const uint64_t *)u->roff.p + kmax, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&flags, d_state + kTsFlags, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&scan_err, u->s.err(), 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (scan_err) return frame_failed(c, u, fail(c, HPN_E_HIP, "prefix-scan hand-off timed out"));
    if (flags || !kmax) return hipSuccess;   // (store_add reads the flags next)
    if ((rc = grow_keep(c, u->norm, (size_t)kStorePad + u->norm_len + total + kStorePad, (size_t)kStorePad + u->norm_len)) != HPN_OK)
        return frame_failed(c, u, rc);
    uint8_t *norm = (uint8_t *)u->norm.p + kStorePad;
    if ((e = launch_kseq_put(d_slot, u->rec.p, (const uint64_t *)u->roff.p, d_state, kmax, fastq ? 1 : 0, norm, u->norm_len, d_desc, c->n_cu, st)) !=
        hipSuccess)
        return e;
    if (!fastq && (e = launch_kseq_fa_copy(d_slot, d_nl, begin, last, L, a, u->rec.p, (const uint64_t *)u->roff.p, norm + u->norm_len, c->n_cu,
                                           st)) != hipSuccess)
        return e;
    u->norm_len += total;
#undef KSEQ_NEED
    return hipSuccess;
}

}  // namespace

namespace hpn {
void kseq_release(hpn_ctx *c)
{
    if (!c->kq) return;
    drop_session(c->kq);
    sort_state_free(c->kq->sorter);
    info_free(c->kq->s);
    delete c->kq;
    c->kq = nullptr;
}
}  // namespace hpn

extern "C" {

int hpn_kseq_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    if (!c->kq) c->kq = new hpn_kseq_state;
    drop_session(c->kq);
    if (!c->kq->sorter && !(c->kq->sorter = sort_state_new(c))) return fail(c, HPN_E_NOMEM, "no memory for the ordering's state");
    const int rc = session_begin(c, c->kq->s, 1, max_bytes);
    if (rc != HPN_OK) return rc;
    HPN_HIP(c, hipMemsetAsync(c->kq->s.d_info, 0, kInfoWords * sizeof(uint32_t), c->stream));   // (the framing's scans flag their errors there)
    return HPN_OK;
}

int hpn_kseq_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_kseq_state *u = c->kq;
    if (u && u->s.open && !u->s.finished && !u->s.m[0].closed && u->shape == HPN_KSEQ_NONE && nbytes && text) {
        // the stream's first byte says which shape the framing holds the stream to
        uint8_t b = 0;
        HPN_HIP(c, hipSetDevice(c->device));
        HPN_HIP(c, hipMemcpy(&b, text, 1, hipMemcpyDefault));
        if (b == '>') u->shape = HPN_KSEQ_FASTA;
        else if (b == '@') u->shape = HPN_KSEQ_FASTQ;
        else {   // text in front of the first header (kseq_read skips it)
            memset(info, 0, sizeof *info);
            info->irregular = HPN_TEXT_KSEQ;
            u->s.open = false;
            return HPN_OK;
        }
    }
    if (u && u->s.open && !u->s.finished && !u->s.m[0].closed && u->s.m[0].len - u->s.m[0].pos + nbytes >= (1ull << 31) - 4096) {
        // an unfinished record beyond what one framing call spans: no regular record is that long
        memset(info, 0, sizeof *info);
        info->irregular = HPN_TEXT_KSEQ;
        u->s.open = false;
        return HPN_OK;
    }
    if (u) u->ctx = c, u->frame_rc = HPN_OK;
    const int rc = session_add(c, u ? &u->s : nullptr, "hpn_kseq", 0, kSortDescBytes, kseq_frame, u, 1u, text, nbytes, last, false, info);
    if (u && u->frame_rc != HPN_OK) {   // the chunk is stored but not framed: the session cannot go on
        u->s.open = false;
        return fail(c, u->frame_rc, "%s", u->frame_err);
    }
    return rc;
}

int hpn_kseq_finish(hpn_ctx *c, hpn_kseq_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_kseq_state *u = c->kq;
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_kseq", kSortDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    RecordStore &m = u->s.m[0];
    if (m.pos < m.len) {   // (the framing consumes every byte of a closed regular stream)
        u->s.open = false;
        return fail(c, HPN_E_STATE, "%llu bytes of the stream are unframed", (unsigned long long)(m.len - m.pos));
    }
    const uint32_t N = (uint32_t)m.n;
    const int fastq = u->shape == HPN_KSEQ_FASTQ;
    res->n_records = N, res->shape = u->shape, res->one_length = 1;
    u->out_total = 0;
    if (!N) {
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->s.finished = true;
        return HPN_OK;
    }
    if ((rc = grow_keep(c, u->norm, 2 * kStorePad, 0)) != HPN_OK) return rc;
    const uint8_t *text = (const uint8_t *)u->norm.p + kStorePad;
    const void *desc = m.desc.p;
    const uint32_t *order = nullptr;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTally], c->stream));
    if ((rc = sort_state_order(c, u->sorter, text, desc, N, &res->rounds, &res->refined, &order)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTally], c->stream));
    c->ev_valid[kFamTally] = true;
    // the heads of the runs, the lengths, the picked records and their sizes
    if ((rc = need(c, u->head, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->at, ((size_t)N + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->pick, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->size, (size_t)N * 4)) != HPN_OK ||
        (rc = need(c, u->off, ((size_t)N + 1) * 8)) != HPN_OK || (rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_kseq_heads(text, desc, order, N, (uint32_t *)u->head.p, u->s.d_info + kKiOther, c->stream));
    HPN_HIP(c, uniq_scan32((const uint32_t *)u->head.p, (uint32_t *)u->at.p, N, (u64 *)u->status.p, u->s.ticket(), u->s.err(), c->stream));
    uint32_t distinct = 0;
    HPN_HIP(c, hipMemcpyAsync(&distinct, (const uint32_t *)u->at.p + N, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = info_fetch(c, u->s)) != HPN_OK) return rc;
    res->n_distinct = distinct;
    SortDesc d0;
    HPN_HIP(c, hipMemcpy(&d0, desc, sizeof d0, hipMemcpyDeviceToHost));
    res->first_len = d0.slen;
    const uint32_t other = u->s.h_info[kKiOther];
    if (other != 0xffffffffu) {
        SortDesc d1;
        HPN_HIP(c, hipMemcpy(&d1, (const SortDesc *)desc + other, sizeof d1, hipMemcpyDeviceToHost));
        res->one_length = 0, res->other_len = d1.slen;
    }
    HPN_HIP(c, launch_kseq_pick(desc, order, (const uint32_t *)u->head.p, (const uint32_t *)u->at.p, N, fastq, (uint32_t *)u->pick.p,
                                (uint32_t *)u->size.p, c->stream));
    uint64_t total = 0;
    if ((rc = scan_sizes(c, u->s, u->status, u->size, u->off, distinct, &total)) != HPN_OK) return rc;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, launch_kseq_write(text, desc, (const uint32_t *)u->pick.p, (const uint64_t *)u->off.p, distinct, fastq, (uint8_t *)u->out.p, c->n_cu,
                                 c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->out_total = res->out_bytes = total;
    u->s.finished = true;
    return HPN_OK;
}

int hpn_kseq_write(hpn_ctx *c, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_kseq_state *u = c->kq;
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_kseq", written);
    return rc != HPN_OK ? rc : session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

}  // extern "C"
