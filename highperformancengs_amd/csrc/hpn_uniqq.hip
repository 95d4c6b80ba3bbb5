// hpn_uniqq.hip -- C ABI of duplicate removal that keeps every quality line (gzfastq_uniqQ.c): hpn_fastq_uniqq_begin / _add /
// _finish / _write.  Kernels: kernels/fastq_uniqq.hip; the store (hpn_store.hpp) and the grouping stage (hpn_uniq_group.hpp) are
// those of hpn_fastq_uniq_*, run over a single-end session of its own.
//
// The reference only ever calls dictAdd, never dictReplace, so its table has the smallest power of two >= max(U, 4) slots: the
// extra doubling of hpn_uniq_group.hpp cannot happen (replace_doubles = false).
#include "hpn_uniq_group.hpp"

namespace hpn {
// kernels/fastq_uniqq.hip
hipError_t launch_uniqq_len(const void *d_desc, const uint32_t *d_order, const uint32_t *d_flag, const uint32_t *d_gid,
                            const uint32_t *d_count, uint32_t n, uint32_t *d_len, uint32_t *d_start, uint32_t *d_max_count, hipStream_t st);
hipError_t launch_uniqq_sizes(const void *d_desc, const uint32_t *d_order, const uint32_t *d_list, const uint32_t *d_start,
                              const uint32_t *d_count, const uint64_t *d_P, uint32_t n_groups, uint64_t *d_total, hipStream_t st);
hipError_t launch_uniqq_base(const void *d_desc, const uint32_t *d_order, const uint32_t *d_list, const uint32_t *d_start,
                             const uint32_t *d_count, const uint64_t *d_P, const uint64_t *d_goff, uint32_t n_groups, uint64_t *d_base,
                             hipStream_t st);
hipError_t launch_uniqq_count_key(const uint32_t *d_list_table, const uint32_t *d_count, uint32_t n_groups, uint64_t *d_key, uint32_t *d_val,
                                  hipStream_t st);
hipError_t launch_uniqq_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_order, const uint32_t *d_flag,
                              const uint32_t *d_gid, const uint32_t *d_count, const uint64_t *d_P, const uint64_t *d_base, uint32_t n,
                              uint8_t *d_out, int n_cu, hipStream_t st);
}  // namespace hpn

using namespace hpn;

struct hpn_uniqq_work {   // what a new session must not inherit
    Scratch len, P, start, total, goff, base, list_count;
    bool have_count_list = false;
    uint32_t max_count = 0;
};

struct hpn_uniqq_state : FamilyState, hpn_uniqq_work {
    static constexpr int kSlot = kStUniqq;
    hpn_uniq_state g;   // single-end: the store, the grouping stage's arrays, the output text
};

namespace {

void drop_session(hpn_uniqq_state *q)
{
    uniq_drop_session(&q->g);
    static_cast<hpn_uniqq_work &>(*q) = hpn_uniqq_work();
}

// -C: count descending, equal counts in the order of the table walk -- one stable sort over the digits of the count that can
// differ (the walk's positions in the low word are ascending as they stand)
int count_list(hpn_ctx *c, hpn_uniqq_state *q)
{
    if (q->have_count_list) return HPN_OK;
    hpn_uniq_state *u = &q->g;
    const uint32_t U = u->U;
    int rc;
    if ((rc = need(c, q->list_count, (size_t)U * 4)) != HPN_OK) return rc;
    uint64_t *key = (uint64_t *)u->key.p;
    uint32_t *val = (uint32_t *)u->val.p;
    int count_bits = 0;
    while (count_bits < 32 && (q->max_count >> count_bits)) ++count_bits;
    HPN_HIP(c, launch_uniqq_count_key((const uint32_t *)u->list_table.p, (const uint32_t *)u->count.p, U, key, val, c->stream));
    if ((rc = uniq_sort(c, u, key, val, U, 32, 32 + count_bits)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(q->list_count.p, val, (size_t)U * 4, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    q->have_count_list = true;
    return HPN_OK;
}

// every group's offset in the output `which` (q->goff, q->base); *total: the output's bytes
int place_groups(hpn_ctx *c, hpn_uniqq_state *q, int which, uint64_t *total)
{
    hpn_uniq_state *u = &q->g;
    const uint32_t U = u->U;
    int rc;
    if (which == HPN_UNIQQ_COUNT_ORDER && (rc = count_list(c, q)) != HPN_OK) return rc;
    const uint32_t *list = (const uint32_t *)(which == HPN_UNIQQ_COUNT_ORDER ? q->list_count.p : u->list_key.p);
    if ((rc = need(c, q->total, (size_t)U * 8)) != HPN_OK || (rc = need(c, q->goff, ((size_t)U + 1) * 8)) != HPN_OK ||
        (rc = need(c, q->base, (size_t)U * 8)) != HPN_OK || (rc = need(c, u->status, uniq_scan_tiles(U) * 8)) != HPN_OK)
        return rc;
    const uint32_t *order = (const uint32_t *)u->order.p, *start = (const uint32_t *)q->start.p, *count = (const uint32_t *)u->count.p;
    const uint64_t *P = (const uint64_t *)q->P.p;
    HPN_HIP(c, launch_uniqq_sizes(u->s.m[0].desc.p, order, list, start, count, P, U, (uint64_t *)q->total.p, c->stream));
    HPN_HIP(c, uniq_scan64w((const uint64_t *)q->total.p, (uint64_t *)q->goff.p, U, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(),
                            c->stream));
    HPN_HIP(c, launch_uniqq_base(u->s.m[0].desc.p, order, list, start, count, P, (const uint64_t *)q->goff.p, U, (uint64_t *)q->base.p, c->stream));
    HPN_HIP(c, hipMemcpyAsync(total, (const uint64_t *)q->goff.p + U, 8, hipMemcpyDeviceToHost, c->stream));
    return u->s.info.fetch(c);
}

// the whole text of one output on the device (u->out, u->out_total bytes)
int build_output(hpn_ctx *c, hpn_uniqq_state *q, int which)
{
    hpn_uniq_state *u = &q->g;
    int rc;
    uint64_t total = 0;
    u->cached_which = -1;
    if ((rc = place_groups(c, q, which, &total)) != HPN_OK) return rc;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_uniqq_write((const uint8_t *)u->s.m[0].store.p + kStorePad, u->s.m[0].desc.p, (const uint32_t *)u->order.p,
                                  (const uint32_t *)u->flag.p, (const uint32_t *)u->gid.p, (const uint32_t *)u->count.p, (const uint64_t *)q->P.p,
                                  (const uint64_t *)q->base.p, u->N, (uint8_t *)u->out.p, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    u->out_total = total;
    u->cached_which = which;
    return HPN_OK;
}

}  // namespace

extern "C" {

int hpn_fastq_uniqq_begin(hpn_ctx *c, uint64_t max_bytes, uint32_t hash_bits)
{
    if (!c) return HPN_E_ARG;
    if (hash_bits > 63) return fail(c, HPN_E_ARG, "hash_bits %u (0 = all 64, or 1 .. 63)", hash_bits);
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniqq_state *q = state_make<hpn_uniqq_state>(c);
    drop_session(q);
    return uniq_begin(c, &q->g, 0, max_bytes, hash_bits);
}

int hpn_fastq_uniqq_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_uniqq_state *q = state<hpn_uniqq_state>(c);
    return session_add(c, q ? &q->g.s : nullptr, "hpn_fastq_uniqq", 0, kUniqDescBytes, frame_by<launch_uniqq_keys>, nullptr, 4u, text, nbytes, last, false, info);
}

int hpn_fastq_uniqq_finish(hpn_ctx *c, hpn_uniqq_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_uniqq_state *q = state<hpn_uniqq_state>(c);
    hpn_uniq_state *u = q ? &q->g : nullptr;
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_fastq_uniqq", kUniqDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    const uint32_t N = u->N = (uint32_t)u->s.m[0].n;
    res->n_records = N;
    if ((rc = uniq_group(c, u, false, &res->hash_size, &res->hash_clashes)) != HPN_OK) return rc;
    const uint32_t U = u->U;
    res->n_unique = U;
    // every sorted position's quality bytes and their 64-bit scan; where each group starts; the greatest count
    if ((rc = need(c, q->len, (size_t)N * 4)) != HPN_OK || (rc = need(c, q->P, ((size_t)N + 1) * 8)) != HPN_OK ||
        (rc = need(c, q->start, (size_t)U * 4)) != HPN_OK || (rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, launch_uniqq_len(u->s.m[0].desc.p, (const uint32_t *)u->order.p, (const uint32_t *)u->flag.p, (const uint32_t *)u->gid.p,
                                (const uint32_t *)u->count.p, N, (uint32_t *)q->len.p, (uint32_t *)q->start.p, u->s.info.d + kUiMaxCount, c->stream));
    HPN_HIP(c, uniq_scan64((const uint32_t *)q->len.p, (uint64_t *)q->P.p, N, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    res->max_count = q->max_count = u->s.info.h[kUiMaxCount];
    if ((rc = place_groups(c, q, HPN_UNIQQ_KEY_ORDER, &res->out_bytes)) != HPN_OK) return rc;   // (both orders hold the same groups)
    u->s.finished = true;
    return HPN_OK;
}

int hpn_fastq_uniqq_write(hpn_ctx *c, int which, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_uniqq_state *q = state<hpn_uniqq_state>(c);
    hpn_uniq_state *u = q ? &q->g : nullptr;
    int rc;
    if ((rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_fastq_uniqq", written)) != HPN_OK) return rc;
    if (which != HPN_UNIQQ_KEY_ORDER && which != HPN_UNIQQ_COUNT_ORDER) return fail(c, HPN_E_ARG, "unknown output %d", which);
    if (u->cached_which != which && (rc = build_output(c, q, which)) != HPN_OK) return rc;
    return session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

}  // extern "C"
