// hpn_pair.hip -- C ABI of the pair splitter (pick_pair.c): hpn_fastq_pair_begin / _add / _finish / _write.  Kernels:
// kernels/fastq_pair.hip, the framing of kernels/fastq_sort.hip (k_sort_frame, as it is), the 64-bit scan of
// kernels/fastq_uniq.hip, the line index of kernels/fastq_text.hip.  The store and its framing in place: hpn_store.hpp.
//
// Two stores, one per mate, each with one SortDesc per record.  _finish proposes a pairing -- the identity when both files hold
// the same number of records, else (or when that does not verify) the join -- and verifies it against the reference's walk
// record by record; a pairing that verifies is written out as four flat texts.  When neither does, the device has no answer:
// HPN_E_DOMAIN with result->unverified, and the caller walks the files as the reference does.
#include "hpn_store.hpp"
#include "kernels/sort_desc.hpp"

namespace hpn {
// kernels/fastq_pair.hip
hipError_t launch_pair_klen(const uint8_t *d_text, const void *d_desc, uint32_t n, uint32_t *d_klen, hipStream_t st);
hipError_t launch_pair_identity(uint32_t n, uint32_t *d_m, hipStream_t st);
hipError_t launch_pair_find(const uint8_t *d_text_a, const void *d_desc_a, const uint32_t *d_klen, uint32_t n_a, const uint8_t *d_text_b,
                            const void *d_desc_b, uint32_t n_b, uint32_t *d_m, int n_cu, hipStream_t st);
hipError_t launch_pair_flags(const uint32_t *d_m, uint32_t n_a, uint32_t n_b, uint32_t *d_flag_a, uint32_t *d_flag_b, hipStream_t st);
hipError_t launch_pair_scatter(const uint32_t *d_m, const uint64_t *d_rank_a, uint32_t n_a, uint32_t *d_pair_a, uint32_t *d_pair_b, hipStream_t st);
hipError_t launch_pair_verify(const uint8_t *d_text_a, const void *d_desc_a, const uint32_t *d_klen, uint32_t n_a, const uint8_t *d_text_b,
                              const void *d_desc_b, uint32_t n_b, const uint32_t *d_m, const uint64_t *d_rank_a, const uint32_t *d_flag_b,
                              const uint64_t *d_rank_b, const uint32_t *d_pair_a, const uint32_t *d_pair_b, uint32_t *d_fail, int n_cu,
                              hipStream_t st);
hipError_t launch_pair_sizes(const void *d_desc, const uint32_t *d_flag, uint32_t n, uint32_t *d_pe, uint32_t *d_se, hipStream_t st);
hipError_t launch_pair_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_flag, const uint64_t *d_off_pe, const uint64_t *d_off_se,
                             uint32_t n, uint8_t *d_out_pe, uint8_t *d_out_se, int n_cu, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
enum { kPrFail = kInfoOwn };   // the family's word of the info block
}  // namespace

struct hpn_pair_work {   // what a new session must not inherit
    Scratch klen, mate, flag[2], rank[2], pair[2], size[2], off[2], status, out[4];
    uint64_t out_total[4] = {0, 0, 0, 0};
};

struct hpn_pair_state : FamilyState, hpn_pair_work {
    static constexpr int kSlot = kStPair;
    StoreSession s;
};

namespace {

void drop_session(hpn_pair_state *u)
{
    session_drop(u->s);
    static_cast<hpn_pair_work &>(*u) = hpn_pair_work();
}

// flags, ranks, the pair list and the one comparison per record over the proposal in u->mate.  *bad: 0xffffffff when the
// proposal is what the walk produces, else the smallest failing mate << 31 | ordinal.
int verify(hpn_ctx *c, hpn_pair_state *u, uint32_t nA, uint32_t nB, uint64_t *n_pairs, uint32_t *bad)
{
    uint32_t *fl[2] = {(uint32_t *)u->flag[0].p, (uint32_t *)u->flag[1].p};
    uint64_t *rk[2] = {(uint64_t *)u->rank[0].p, (uint64_t *)u->rank[1].p};
    const uint32_t n[2] = {nA, nB};
    HPN_HIP(c, launch_pair_flags((const uint32_t *)u->mate.p, nA, nB, fl[0], fl[1], c->stream));
    for (int s = 0; s < 2; ++s) {
        if (n[s]) HPN_HIP(c, uniq_scan64(fl[s], rk[s], n[s], (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
        else HPN_HIP(c, hipMemsetAsync(rk[s], 0, 8, c->stream));
    }
    HPN_HIP(c, launch_pair_scatter((const uint32_t *)u->mate.p, rk[0], nA, (uint32_t *)u->pair[0].p, (uint32_t *)u->pair[1].p, c->stream));
    HPN_HIP(c, launch_pair_verify(u->s.text(0), u->s.m[0].desc.p, (const uint32_t *)u->klen.p, nA, u->s.text(1), u->s.m[1].desc.p, nB,
                                  (const uint32_t *)u->mate.p, rk[0], fl[1], rk[1], (const uint32_t *)u->pair[0].p, (const uint32_t *)u->pair[1].p,
                                  u->s.info.d + kPrFail, c->n_cu, c->stream));
    HPN_HIP(c, hipMemcpyAsync(n_pairs, rk[0] + nA, 8, hipMemcpyDeviceToHost, c->stream));
    const int rc = u->s.info.fetch(c);
    *bad = u->s.info.h[kPrFail];
    return rc;
}

}  // namespace

extern "C" {

int hpn_fastq_pair_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_pair_state *u = state_make<hpn_pair_state>(c);
    drop_session(u);
    return session_begin(c, u->s, 2, max_bytes);
}

int hpn_fastq_pair_add(hpn_ctx *c, int mate, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_pair_state *u = state<hpn_pair_state>(c);
    return session_add(c, u ? &u->s : nullptr, "hpn_fastq_pair", mate, kSortDescBytes, frame_by<launch_sort_frame>, nullptr, 4u, text, nbytes, last, true, info);
}

int hpn_fastq_pair_finish(hpn_ctx *c, hpn_pair_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_pair_state *u = state<hpn_pair_state>(c);
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_fastq_pair", kSortDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    res->fail_record = -1;
    const uint32_t nA = (uint32_t)u->s.m[0].n, nB = (uint32_t)u->s.m[1].n, n[2] = {nA, nB};
    const uint32_t big = nA > nB ? nA : nB;
    res->n_records[0] = nA, res->n_records[1] = nB;
    if (!nA && !nB) {   // the walk's first round finds nothing: four empty outputs
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->s.finished = true;
        return HPN_OK;
    }
    if ((rc = need(c, u->klen, (size_t)nA * 4)) != HPN_OK || (rc = need(c, u->mate, (size_t)nA * 4)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(big) * 8)) != HPN_OK)
        return rc;
    for (int s = 0; s < 2; ++s)
        if ((rc = need(c, u->flag[s], (size_t)n[s] * 4)) != HPN_OK || (rc = need(c, u->rank[s], ((size_t)n[s] + 1) * 8)) != HPN_OK ||
            (rc = need(c, u->pair[s], (size_t)nA * 4)) != HPN_OK)   // (a join may give several A records one mate)
            return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_pair_klen(u->s.text(0), u->s.m[0].desc.p, nA, (uint32_t *)u->klen.p, c->stream));
    uint64_t n_pairs = 0;
    uint32_t bad = 0;
    bool ok = false;
    if (nA == nB) {   // every read still has its mate, in any order: the common case
        HPN_HIP(c, launch_pair_identity(nA, (uint32_t *)u->mate.p, c->stream));
        if ((rc = verify(c, u, nA, nB, &n_pairs, &bad)) != HPN_OK) return rc;
        ok = bad == 0xffffffffu;
        res->route = HPN_PAIR_IDENTITY;
    }
    if (!ok) {
        HPN_HIP(c, launch_pair_find(u->s.text(0), u->s.m[0].desc.p, (const uint32_t *)u->klen.p, nA, u->s.text(1), u->s.m[1].desc.p, nB,
                                    (uint32_t *)u->mate.p, c->n_cu, c->stream));
        if ((rc = verify(c, u, nA, nB, &n_pairs, &bad)) != HPN_OK) return rc;
        ok = bad == 0xffffffffu;
        res->route = HPN_PAIR_JOIN;
    }
    if (!ok) {
        res->unverified = 1, res->fail_mate = bad >> 31, res->fail_record = (int64_t)(bad & 0x7fffffffu);
        drop_session(u);
        return fail(c, HPN_E_DOMAIN, "neither pairing is the walk's: record %u (0-based) of mate %u does not verify", bad & 0x7fffffffu, bad >> 31);
    }
    res->n_pairs = n_pairs, res->n_single[0] = nA - n_pairs, res->n_single[1] = nB - n_pairs;
    // the outputs, a mate at a time: sizes in two columns, two scans, one writer
    for (int s = 0; s < 2; ++s) {
        if (!n[s]) continue;
        for (int col = 0; col < 2; ++col)
            if ((rc = need(c, u->size[col], (size_t)big * 4)) != HPN_OK || (rc = need(c, u->off[col], ((size_t)big + 1) * 8)) != HPN_OK) return rc;
        const uint64_t *of[2] = {(const uint64_t *)u->off[0].p, (const uint64_t *)u->off[1].p};
        HPN_HIP(c, launch_pair_sizes(u->s.m[s].desc.p, (const uint32_t *)u->flag[s].p, n[s], (uint32_t *)u->size[0].p, (uint32_t *)u->size[1].p, c->stream));
        uint64_t sum[2] = {0, 0};
        for (int col = 0; col < 2; ++col)
            if ((rc = scan_sizes(c, u->s.info, u->status, u->size[col], u->off[col], n[s], &sum[col])) != HPN_OK) return rc;
        for (int col = 0; col < 2; ++col) {
            if ((rc = need(c, u->out[2 * s + col], sum[col])) != HPN_OK) return rc;
            u->out_total[2 * s + col] = res->out_bytes[2 * s + col] = sum[col];
        }
        HPN_HIP(c, launch_pair_write(u->s.text(s), u->s.m[s].desc.p, (const uint32_t *)u->flag[s].p, of[0], of[1], n[s],
                                     (uint8_t *)u->out[2 * s].p, (uint8_t *)u->out[2 * s + 1].p, c->n_cu, c->stream));
    }
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    u->s.finished = true;
    return HPN_OK;
}

int hpn_fastq_pair_write(hpn_ctx *c, int which_output, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_pair_state *u = state<hpn_pair_state>(c);
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_fastq_pair", written);
    if (rc != HPN_OK) return rc;
    if (which_output < 0 || which_output > 3) return fail(c, HPN_E_ARG, "which_output is %d (0 .. 3)", which_output);
    return session_write_slice(c, u->out[which_output], u->out_total[which_output], offset, out, cap, written);
}

}  // extern "C"
