// hpn_kseq.hip -- C ABI of map_kseq.cpp / kbtree_kseq.c: hpn_kseq_begin / _add / _finish / _write.
// Kernels: kernels/kseq_frame.hip (the framing, the heads of the runs, the writer), the refinement sort of kernels/fastq_sort.hip
// in its third key mode (hpn_sorter.hpp: order_records), the scans of kernels/fastq_uniq.hip, the line index of
// kernels/fastq_text.hip.  The stream lies in the session's store (hpn_store.hpp) and is framed chunk by chunk, an unfinished
// record staying unframed; what is framed is copied into a second, NORMALISED store -- "name comment\nsequence\n[quality]" per
// record, the sequence's lines joined -- which the descriptors (SortDesc) point into and everything behind the framing reads.
#include "hpn_sorter.hpp"
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
}  // namespace hpn

using namespace hpn;

namespace {
enum { kKiOther = kInfoOwn };   // the family's word of the info block: the first record whose length is not the first record's
}

struct hpn_kseq_work {   // what a new session must not inherit
    Scratch norm;          // kStorePad, the normalised records, kStorePad
    uint64_t norm_len = 0;
    uint32_t shape = HPN_KSEQ_NONE;
    Scratch l_hdr, l_t, l_ne, l_hid, l_P, l_NE, l_hline, l_x, rec, rsize, roff, status;   // the framing's arrays, per chunk
    Scratch head, at, pick, size, off, out;                                               // _finish
    uint64_t out_total = 0;
};

struct hpn_kseq_state : FamilyState, hpn_kseq_work {
    static constexpr int kSlot = kStKseq;
    StoreSession s;        // m[0]: the stream as it came; its descriptors point into `norm`
    Sorter sorter;
};

namespace {

void drop_session(hpn_kseq_state *u)
{
    session_drop(u->s);
    static_cast<hpn_kseq_work &>(*u) = hpn_kseq_work();
    u->sorter.drop();
}

// The chunk's records into the normalised store and their descriptors (store_frame_fn).  max_records is the chunk's line count.
int kseq_frame(hpn_ctx *c, const FrameArgs &f)
{
    hpn_kseq_state *u = (hpn_kseq_state *)f.user;
    hipStream_t st = c->stream;
    const uint32_t L = f.max_records;
    const bool fastq = u->shape == HPN_KSEQ_FASTQ;
    const uint32_t kmax = fastq ? L / 4u : (L + 1u) / 2u;
    uint32_t *ticket = u->s.info.ticket(), *err = u->s.info.err();
    int rc;
    if ((rc = need(c, u->rec, ((size_t)kmax + 1) * kKseqRecBytes)) != HPN_OK || (rc = need(c, u->rsize, ((size_t)kmax + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->roff, ((size_t)kmax + 2) * 8)) != HPN_OK || (rc = need(c, u->status, uniq_scan_tiles((uint64_t)L + 1) * 8)) != HPN_OK)
        return rc;
    KseqLines a = {};
    if (fastq) {
        HPN_HIP(c, launch_kseq_fq_recs(f.d_slot, f.d_nl, f.begin, f.end, f.last, L, u->rec.p, (uint32_t *)u->rsize.p, f.d_state, st));
    } else {
        Scratch *per[] = {&u->l_hdr, &u->l_t, &u->l_ne, &u->l_hid, &u->l_P, &u->l_NE, &u->l_hline, &u->l_x};
        for (Scratch *s : per)
            if ((rc = need(c, *s, ((size_t)L + 2) * 4)) != HPN_OK) return rc;
        a = KseqLines{(uint32_t *)u->l_hdr.p, (uint32_t *)u->l_t.p,  (uint32_t *)u->l_ne.p,    (uint32_t *)u->l_hid.p,
                      (uint32_t *)u->l_P.p,   (uint32_t *)u->l_NE.p, (uint32_t *)u->l_hline.p, (uint32_t *)u->l_x.p};
        u64 *status = (u64 *)u->status.p;
        HPN_HIP(c, launch_kseq_fa_lines(f.d_slot, f.d_nl, f.begin, L, a, f.d_state, st));
        HPN_HIP(c, uniq_scan32(a.hdr, a.hid, L, status, ticket, err, st));
        HPN_HIP(c, uniq_scan32(a.t, a.P, L, status, ticket, err, st));
        HPN_HIP(c, uniq_scan32(a.ne, a.NE, L, status, ticket, err, st));
        HPN_HIP(c, launch_kseq_fa_recs(f.d_slot, f.d_nl, f.begin, f.end, f.last, L, a, u->rec.p, (uint32_t *)u->rsize.p, f.d_state, st));
    }
    HPN_HIP(c, uniq_scan64((const uint32_t *)u->rsize.p, (uint64_t *)u->roff.p, kmax, (u64 *)u->status.p, ticket, err, st));
    // the chunk's bytes in the normalised store, and whether the chunk is regular at all: both on the host before the copies
    uint64_t total = 0;
    uint32_t flags = 0, scan_err = 0;
    HPN_HIP(c, hipMemcpyAsync(&total, (const uint64_t *)u->roff.p + kmax, 8, hipMemcpyDeviceToHost, st));
    HPN_HIP(c, hipMemcpyAsync(&flags, f.d_state + kTsFlags, 4, hipMemcpyDeviceToHost, st));
    HPN_HIP(c, hipMemcpyAsync(&scan_err, err, 4, hipMemcpyDeviceToHost, st));
    HPN_HIP(c, hipStreamSynchronize(st));
    if (scan_err) return fail(c, HPN_E_HIP, "prefix-scan hand-off timed out");
    if (flags || !kmax) return HPN_OK;   // (store_add reads the flags next)
    if ((rc = grow_keep(c, u->norm, (size_t)kStorePad + u->norm_len + total + kStorePad, (size_t)kStorePad + u->norm_len)) != HPN_OK) return rc;
    uint8_t *norm = (uint8_t *)u->norm.p + kStorePad;
    HPN_HIP(c, launch_kseq_put(f.d_slot, u->rec.p, (const uint64_t *)u->roff.p, f.d_state, kmax, fastq ? 1 : 0, norm, u->norm_len, f.d_desc, c->n_cu, st));
    if (!fastq)
        HPN_HIP(c, launch_kseq_fa_copy(f.d_slot, f.d_nl, f.begin, f.last, L, a, u->rec.p, (const uint64_t *)u->roff.p, norm + u->norm_len, c->n_cu, st));
    u->norm_len += total;
    return HPN_OK;
}

}  // namespace

extern "C" {

int hpn_kseq_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_kseq_state *u = state_make<hpn_kseq_state>(c);
    drop_session(u);
    u->sorter.bytes_only = 1;
    const int rc = session_begin(c, u->s, 1, max_bytes);
    return rc != HPN_OK ? rc : u->s.info.zero(c);   // (the framing's scans flag their errors there)
}

int hpn_kseq_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_kseq_state *u = state<hpn_kseq_state>(c);
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
    return session_add(c, u ? &u->s : nullptr, "hpn_kseq", 0, kSortDescBytes, kseq_frame, u, 1u, text, nbytes, last, false, info);
}

int hpn_kseq_finish(hpn_ctx *c, hpn_kseq_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_kseq_state *u = state<hpn_kseq_state>(c);
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
    hpn_sort_result sorted = {};
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTally], c->stream));
    rc = order_records(c, &u->sorter, text, desc, N, &sorted);
    res->rounds = sorted.rounds, res->refined = sorted.refined;
    if (rc != HPN_OK) return rc;
    const uint32_t *order = (const uint32_t *)u->sorter.order.p;
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTally], c->stream));
    c->ev_valid[kFamTally] = true;
    // the heads of the runs, the lengths, the picked records and their sizes
    if ((rc = need(c, u->head, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->at, ((size_t)N + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->pick, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->size, (size_t)N * 4)) != HPN_OK ||
        (rc = need(c, u->off, ((size_t)N + 1) * 8)) != HPN_OK || (rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_kseq_heads(text, desc, order, N, (uint32_t *)u->head.p, u->s.info.d + kKiOther, c->stream));
    HPN_HIP(c, uniq_scan32((const uint32_t *)u->head.p, (uint32_t *)u->at.p, N, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
    uint32_t distinct = 0;
    HPN_HIP(c, hipMemcpyAsync(&distinct, (const uint32_t *)u->at.p + N, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    res->n_distinct = distinct;
    SortDesc d0;
    HPN_HIP(c, hipMemcpy(&d0, desc, sizeof d0, hipMemcpyDeviceToHost));
    res->first_len = d0.slen;
    const uint32_t other = u->s.info.h[kKiOther];
    if (other != 0xffffffffu) {
        SortDesc d1;
        HPN_HIP(c, hipMemcpy(&d1, (const SortDesc *)desc + other, sizeof d1, hipMemcpyDeviceToHost));
        res->one_length = 0, res->other_len = d1.slen;
    }
    HPN_HIP(c, launch_kseq_pick(desc, order, (const uint32_t *)u->head.p, (const uint32_t *)u->at.p, N, fastq, (uint32_t *)u->pick.p,
                                (uint32_t *)u->size.p, c->stream));
    uint64_t total = 0;
    if ((rc = scan_sizes(c, u->s.info, u->status, u->size, u->off, distinct, &total)) != HPN_OK) return rc;
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
    hpn_kseq_state *u = state<hpn_kseq_state>(c);
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_kseq", written);
    return rc != HPN_OK ? rc : session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

}  // extern "C"
