// hpn_pair.hip -- C ABI of the pair splitter (pick_pair.c): hpn_fastq_pair_begin / _add / _finish / _write.  Kernels:
// kernels/fastq_pair.hip, the framing of kernels/fastq_sort.hip (k_sort_frame, as it is), the 64-bit scan of
// kernels/fastq_uniq.hip, the line index of kernels/fastq_text.hip.  The store and its framing in place: hpn_store.hpp.
//
// Two stores, one per mate, each with one SortDesc per record.  _finish proposes a pairing -- the identity when both files hold
// the same number of records, else (or when that does not verify) the join -- and verifies it against the reference's walk
// record by record; a pairing that verifies is written out as four flat texts.  When neither does, the device has no answer:
// HPN_E_DOMAIN with result->unverified, and the caller walks the files as the reference does.
#include <string.h>

#include "hpn_store.hpp"

namespace hpn {
// kernels/fastq_sort.hip
hipError_t launch_sort_frame(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                             void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st);
// kernels/fastq_uniq.hip
hipError_t uniq_scan64(const uint32_t *d_in, uint64_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st);
uint64_t uniq_scan_tiles(uint64_t n);
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
constexpr size_t kDescBytes = 16;                                       // kernels/fastq_sort.hip: SortDesc
enum { kPrTicket = 0, kPrErr = 1, kPrFail = 2, kPrWords = 4 };          // the device's info block (uint32 words)
}  // namespace

struct hpn_pair_state {
    uint64_t limit = 0;
    bool open = false, finished = false;
    RecordStore m[2];
    Scratch klen, mate, flag[2], rank[2], pair[2], size[2], off[2], status, out[4];
    uint32_t *d_info = nullptr, *h_info = nullptr;
    uint64_t out_total[4] = {0, 0, 0, 0};
};

namespace {

void drop_session(hpn_pair_state *u)
{
    store_release(u->m[0]);
    store_release(u->m[1]);
    Scratch *ss[] = {&u->klen,    &u->mate,    &u->flag[0], &u->flag[1], &u->rank[0], &u->rank[1], &u->pair[0], &u->pair[1], &u->size[0],
                     &u->size[1], &u->off[0],  &u->off[1],  &u->status,  &u->out[0],  &u->out[1],  &u->out[2],  &u->out[3]};
    for (Scratch *s : ss) release_scratch(*s);
    u->open = u->finished = false;
    for (uint64_t &t : u->out_total) t = 0;
}

const uint8_t *text_of(const RecordStore &m) { return (const uint8_t *)m.store.p + kStorePad; }

// flags, ranks, the pair list and the one comparison per record over the proposal in u->mate.  *bad: 0xffffffff when the
// proposal is what the walk produces, else the smallest failing mate << 31 | ordinal.
int verify(hpn_ctx *c, hpn_pair_state *u, uint32_t nA, uint32_t nB, uint64_t *n_pairs, uint32_t *bad)
{
    uint32_t *fl[2] = {(uint32_t *)u->flag[0].p, (uint32_t *)u->flag[1].p};
    uint64_t *rk[2] = {(uint64_t *)u->rank[0].p, (uint64_t *)u->rank[1].p};
    const uint32_t n[2] = {nA, nB};
    HPN_HIP(c, launch_pair_flags((const uint32_t *)u->mate.p, nA, nB, fl[0], fl[1], c->stream));
    for (int s = 0; s < 2; ++s) {
        if (n[s]) HPN_HIP(c, uniq_scan64(fl[s], rk[s], n[s], (u64 *)u->status.p, u->d_info + kPrTicket, u->d_info + kPrErr, c->stream));
        else HPN_HIP(c, hipMemsetAsync(rk[s], 0, 8, c->stream));
    }
    HPN_HIP(c, launch_pair_scatter((const uint32_t *)u->mate.p, rk[0], nA, (uint32_t *)u->pair[0].p, (uint32_t *)u->pair[1].p, c->stream));
    HPN_HIP(c, launch_pair_verify(text_of(u->m[0]), u->m[0].desc.p, (const uint32_t *)u->klen.p, nA, text_of(u->m[1]), u->m[1].desc.p, nB,
                                  (const uint32_t *)u->mate.p, rk[0], fl[1], rk[1], (const uint32_t *)u->pair[0].p, (const uint32_t *)u->pair[1].p,
                                  u->d_info + kPrFail, c->n_cu, c->stream));
    HPN_HIP(c, hipMemcpyAsync(n_pairs, rk[0] + nA, 8, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipMemcpyAsync(u->h_info, u->d_info, kPrWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (u->h_info[kPrErr]) return fail(c, HPN_E_HIP, "prefix-scan hand-off timed out");
    *bad = u->h_info[kPrFail];
    return HPN_OK;
}

}  // namespace

namespace hpn {
void pair_release(hpn_ctx *c)
{
    if (!c->pr) return;
    drop_session(c->pr);
    if (c->pr->d_info) (void)hipFree(c->pr->d_info);
    if (c->pr->h_info) (void)hipHostFree(c->pr->h_info);
    delete c->pr;
    c->pr = nullptr;
}
}  // namespace hpn

extern "C" {

int hpn_fastq_pair_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    if (!c->pr) c->pr = new hpn_pair_state;
    hpn_pair_state *u = c->pr;
    if (!u->d_info) {
        HPN_HIP(c, hipMalloc((void **)&u->d_info, kPrWords * sizeof(uint32_t)));
        HPN_HIP(c, hipHostMalloc((void **)&u->h_info, kPrWords * sizeof(uint32_t), hipHostMallocDefault));
    }
    drop_session(u);
    if (!max_bytes) {   // half of what is free, as hpn_fastq_sort_begin: the other half is the reserve for the stores' growth and the outputs
        size_t fr = 0, total = 0;
        HPN_HIP(c, hipMemGetInfo(&fr, &total));
        max_bytes = fr / 2;
    }
    u->limit = max_bytes;
    u->open = true;
    return HPN_OK;
}

int hpn_fastq_pair_add(hpn_ctx *c, int mate, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_pair_state *u = c->pr;
    if (!u || !u->open || u->finished) return fail(c, HPN_E_STATE, "hpn_fastq_pair_begin first (or the session was closed by an irregular chunk)");
    if (mate != 0 && mate != 1) return fail(c, HPN_E_ARG, "mate is %d (0 or 1)", mate);
    if (nbytes && !text) return fail(c, HPN_E_ARG, "text is NULL");
    RecordStore &m = u->m[mate];
    if (m.closed) return fail(c, HPN_E_STATE, "mate %d's stream has had its last chunk", mate);
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t span = m.len - m.pos + nbytes;
    if (span >= (1ull << 31) - 4096) return fail(c, HPN_E_ARG, "chunk of %llu bytes (limit 2^31 - 4 KiB with the unfinished record)", (unsigned long long)nbytes);
    const uint64_t held = u->m[0].len + u->m[1].len;
    if (held + nbytes > u->limit) {
        u->open = false;
        return fail(c, HPN_E_CAPACITY, "the stores need %llu bytes, max_bytes is %llu", (unsigned long long)(held + nbytes), (unsigned long long)u->limit);
    }
    bool close = false;
    const int rc = store_add(c, m, kDescBytes, launch_sort_frame, text, nbytes, last, &info->n_records, &info->irregular, &close);
    info->store_bytes = m.len;
    if (close) u->open = false;
    return rc;
}

int hpn_fastq_pair_finish(hpn_ctx *c, hpn_pair_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_pair_state *u = c->pr;
    if (!u || !u->open || u->finished) return fail(c, HPN_E_STATE, "no open hpn_fastq_pair session");
    if (!u->m[0].closed || !u->m[1].closed) return fail(c, HPN_E_STATE, "both mates' streams need their last chunk first");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->fail_record = -1;
    int rc;
    const uint32_t nA = (uint32_t)u->m[0].n, nB = (uint32_t)u->m[1].n, n[2] = {nA, nB};
    const uint32_t big = nA > nB ? nA : nB;
    res->n_records[0] = nA, res->n_records[1] = nB;
    if (!nA && !nB) {   // the walk's first round finds nothing: four empty outputs
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->finished = true;
        return HPN_OK;
    }
    if ((rc = need(c, u->klen, (size_t)nA * 4)) != HPN_OK || (rc = need(c, u->mate, (size_t)nA * 4)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(big) * 8)) != HPN_OK)
        return rc;
    for (int s = 0; s < 2; ++s)
        if ((rc = need(c, u->flag[s], (size_t)n[s] * 4)) != HPN_OK || (rc = need(c, u->rank[s], ((size_t)n[s] + 1) * 8)) != HPN_OK ||
            (rc = need(c, u->pair[s], (size_t)nA * 4)) != HPN_OK)   // (a join may give several A records one mate)
            return rc;
    HPN_HIP(c, hipMemsetAsync(u->d_info, 0, kPrWords * sizeof(uint32_t), c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_pair_klen(text_of(u->m[0]), u->m[0].desc.p, nA, (uint32_t *)u->klen.p, c->stream));
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
        HPN_HIP(c, launch_pair_find(text_of(u->m[0]), u->m[0].desc.p, (const uint32_t *)u->klen.p, nA, text_of(u->m[1]), u->m[1].desc.p, nB,
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
        uint32_t *sz[2] = {(uint32_t *)u->size[0].p, (uint32_t *)u->size[1].p};
        uint64_t *of[2] = {(uint64_t *)u->off[0].p, (uint64_t *)u->off[1].p};
        HPN_HIP(c, launch_pair_sizes(u->m[s].desc.p, (const uint32_t *)u->flag[s].p, n[s], sz[0], sz[1], c->stream));
        uint64_t sum[2] = {0, 0};
        for (int col = 0; col < 2; ++col) {
            HPN_HIP(c, uniq_scan64(sz[col], of[col], n[s], (u64 *)u->status.p, u->d_info + kPrTicket, u->d_info + kPrErr, c->stream));
            HPN_HIP(c, hipMemcpyAsync(&sum[col], of[col] + n[s], 8, hipMemcpyDeviceToHost, c->stream));
        }
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        for (int col = 0; col < 2; ++col) {
            if ((rc = need(c, u->out[2 * s + col], sum[col])) != HPN_OK) return rc;
            u->out_total[2 * s + col] = res->out_bytes[2 * s + col] = sum[col];
        }
        HPN_HIP(c, launch_pair_write(text_of(u->m[s]), u->m[s].desc.p, (const uint32_t *)u->flag[s].p, of[0], of[1], n[s],
                                     (uint8_t *)u->out[2 * s].p, (uint8_t *)u->out[2 * s + 1].p, c->n_cu, c->stream));
    }
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    HPN_HIP(c, hipMemcpyAsync(u->h_info, u->d_info, kPrWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (u->h_info[kPrErr]) return fail(c, HPN_E_HIP, "prefix-scan hand-off timed out");
    u->finished = true;
    return HPN_OK;
}

int hpn_fastq_pair_write(hpn_ctx *c, int which_output, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_pair_state *u = c->pr;
    if (!u || !u->finished) return fail(c, HPN_E_STATE, "hpn_fastq_pair_finish first");
    if (which_output < 0 || which_output > 3) return fail(c, HPN_E_ARG, "which_output is %d (0 .. 3)", which_output);
    HPN_HIP(c, hipSetDevice(c->device));
    *written = 0;
    const uint64_t total = u->out_total[which_output];
    if (offset > total) return fail(c, HPN_E_ARG, "offset %llu beyond the output's %llu bytes", (unsigned long long)offset, (unsigned long long)total);
    const uint64_t k = total - offset < cap ? total - offset : cap;
    if (k && !out) return fail(c, HPN_E_ARG, "out is NULL");
    if (k) HPN_HIP(c, hipMemcpyAsync(out, (const uint8_t *)u->out[which_output].p + offset, k, hipMemcpyDefault, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    *written = k;
    return HPN_OK;
}

}  // extern "C"
