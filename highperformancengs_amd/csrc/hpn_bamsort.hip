// hpn_bamsort.hip -- C ABI of samtools' coordinate sort (bam_sort.c): hpn_bam_sort_begin / _add_raw_dev / _finish / _order / _sizes /
// _emit / _blocks / _payload_dev / _stored_dev.  Kernels: kernels/bam_sort.hip; the radix sort and the scan through
// hpn_sort_pairs_u64_bits and hpn_excl_scan (device pointers); the cuts, the CRC-32 and the stored framing: hpn_cuts.hpp.
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch: keys, sizes and checks, and the
// batch's records -- one slice of the inflated stream -- appended to the record store by one copy.  _finish ranks the high words,
// sorts (key, ordinal) over the bits the keys use, and scans the sorted sizes into output offsets.  _emit gathers the next slice of
// the sorted records behind the bytes of the block the slice before left open, cuts it as bam_write1 would, and keeps the last
// block open for the next slice.
#include <string.h>

#include <vector>

#include "hpn_cuts.hpp"
#include "hpn_store.hpp"

namespace hpn {
// kernels/bam_sort.hip
hipError_t launch_bamsort_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, u64 *key, uint32_t *val,
                               uint32_t *size, u64 *soff, u64 *info, hipStream_t st);
hipError_t launch_bamsort_rank(u64 *key, uint64_t n, u64 *info, hipStream_t st);
hipError_t launch_bamsort_psize(const uint32_t *size, const uint32_t *order, uint64_t n, uint32_t *psize, hipStream_t st);
hipError_t launch_bamsort_items(const u64 *out_off, uint64_t first, uint64_t cnt, uint32_t fill, uint32_t open_key, u64 *Q, uint32_t *key, hipStream_t st);
hipError_t launch_bamsort_gather(const uint8_t *store, const u64 *soff, const uint32_t *size, const uint32_t *order, const u64 *out_off, uint64_t first,
                                 uint64_t cnt, uint8_t *pay, int n_cu, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
enum { kBsBad = 0, kBsFirst, kBsEnd, kBsLoMin, kBsLoMax, kBsHiMin, kBsHiMax, kBsMem, kBsMaxKey, kBsWords = 16 };   // kernels/bam_sort.hip
constexpr uint64_t kMaxRecords = (1ull << 31) - 1;     // the sort's contract
}  // namespace

struct hpn_bamsort_work {   // what a new session must not inherit
    Scratch store, key, val, size, soff, psize, out_off, info, cut_info, Q, ikey, pay, keep;
    CutWork cw;
    bool open = false, dead = false, finished = false, ended = false;
    uint64_t records = 0, store_len = 0, payload = 0, emitted = 0;
    uint32_t fill = 0, sort_bits = 0;
    int64_t bad_record = -1;
    int32_t bad_tid = 0, bad_pos = 0;
    uint32_t reason = 0;
    uint64_t fresh_mem = 0;
    std::vector<hpn_split_block> list;   // the closed blocks of the last _emit
    uint64_t payload_bytes = 0, stored_bytes = 0;
    bool stored_made = false;
};

struct hpn_bamsort_state : FamilyState, hpn_bamsort_work {
    static constexpr int kSlot = kStBamSort;
};

namespace {

hpn_bamsort_state *live(hpn_ctx *c, const char *who, bool want_finished)
{
    hpn_bamsort_state *u = state<hpn_bamsort_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "%s before hpn_bam_sort_begin", who), nullptr;
    if (want_finished && !u->finished) return fail(c, HPN_E_STATE, "%s before hpn_bam_sort_finish", who), nullptr;
    if (want_finished && u->dead) return fail(c, HPN_E_STATE, "%s: a record lies outside the domain, nothing was sorted", who), nullptr;
    return u;
}

}  // namespace

extern "C" {

int hpn_bam_sort_begin(hpn_ctx *c)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_bamsort_state *u = state_make<hpn_bamsort_state>(c);
    static_cast<hpn_bamsort_work &>(*u) = hpn_bamsort_work();
    int rc;
    if ((rc = scratch_reserve(c, u->info, kBsWords * sizeof(u64))) != HPN_OK || (rc = scratch_reserve(c, u->cut_info, 64)) != HPN_OK ||
        (rc = scratch_reserve(c, u->keep, kCutFull + 64)) != HPN_OK)
        return rc;
    u64 init[kBsWords] = {0};
    init[kBsBad] = init[kBsLoMin] = init[kBsHiMin] = ~0ull;
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (`init` is this call's)
    u->open = true;
    return HPN_OK;
}

int hpn_bam_sort_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, hpn_bamsort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_add_raw_dev", false);
    if (!u) return HPN_E_STATE;
    if (u->finished) return fail(c, HPN_E_STATE, "hpn_bam_sort_add_raw_dev behind hpn_bam_sort_finish");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t n = d_raw ? c->r_n : 0;
    info->n_records = n, info->store_bytes = u->store_len;
    info->bad_record = u->bad_record, info->bad_tid = u->bad_tid, info->bad_pos = u->bad_pos, info->reason = u->reason;
    if (u->dead || !n) return HPN_OK;
    if (u->records + n > kMaxRecords) {                // the first record the sort cannot take
        u->dead = true;
        u->bad_record = info->bad_record = (int64_t)kMaxRecords, u->reason = info->reason = 3;
        u->records += n;
        return HPN_OK;
    }
    int rc;
    const uint64_t have = u->records, all = have + n;
    if ((rc = grow_keep(c, u->key, all * 8, have * 8)) != HPN_OK || (rc = grow_keep(c, u->val, all * 4, have * 4)) != HPN_OK ||
        (rc = grow_keep(c, u->size, all * 4, have * 4)) != HPN_OK || (rc = grow_keep(c, u->soff, all * 8, have * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, launch_bamsort_keys(d_raw, (const uint64_t *)c->r_off.p, n, have, u->store_len, (u64 *)u->key.p, (uint32_t *)u->val.p, (uint32_t *)u->size.p,
                                   (u64 *)u->soff.p, (u64 *)u->info.p, c->stream));
    u64 h[3];
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (h[kBsBad] != ~0ull) {                          // the first record outside the domain: refID and pos for the message
        const uint64_t ord = h[kBsBad] >> 3;
        uint64_t off = 0;
        int32_t f[2] = {0, 0};
        HPN_HIP(c, hipMemcpyAsync(&off, (const uint64_t *)c->r_off.p + (ord - have), sizeof off, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        HPN_HIP(c, hipMemcpyAsync(f, d_raw + off + 4, sizeof f, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->dead = true;
        u->bad_record = (int64_t)ord, u->bad_tid = f[0], u->bad_pos = f[1], u->reason = (uint32_t)(h[kBsBad] & 7);
        u->records = all;
        info->bad_record = u->bad_record, info->bad_tid = u->bad_tid, info->bad_pos = u->bad_pos, info->reason = u->reason;
        return HPN_OK;
    }
    if (h[kBsEnd] < h[kBsFirst]) return fail(c, HPN_E_HIP, "hpn_bam_sort: the batch's records end at %llu, in front of their start %llu",
                                             (unsigned long long)h[kBsEnd], (unsigned long long)h[kBsFirst]);
    const uint64_t rec_bytes = h[kBsEnd] - h[kBsFirst];
    if ((rc = grow_keep(c, u->store, u->store_len + rec_bytes + 64, u->store_len)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync((uint8_t *)u->store.p + u->store_len, d_raw + h[kBsFirst], rec_bytes, hipMemcpyDeviceToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (the caller's d_raw is free to go)
    u->store_len += rec_bytes, u->records = all;
    info->store_bytes = u->store_len;
    return HPN_OK;
}

int hpn_bam_sort_finish(hpn_ctx *c, hpn_bamsort_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_finish", false);
    if (!u) return HPN_E_STATE;
    if (u->finished) return fail(c, HPN_E_STATE, "hpn_bam_sort_finish twice");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->n_records = u->records;
    res->bad_record = u->bad_record, res->bad_tid = u->bad_tid, res->bad_pos = u->bad_pos, res->reason = u->reason;
    u->finished = true;
    if (u->dead) return HPN_OK;
    const uint64_t n = u->records;
    int rc;
    if ((rc = need(c, u->psize, n * 4)) != HPN_OK || (rc = need(c, u->out_off, (n + 1) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, launch_bamsort_rank((u64 *)u->key.p, n, (u64 *)u->info.p, c->stream));
    u64 h[kBsWords];
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->fresh_mem = h[kBsMem];
    u->sort_bits = 0;
    for (u64 k = h[kBsMaxKey]; k; k >>= 1) ++u->sort_bits;      // bit 0 up to the highest bit set in any key
    if (n > 1 && u->sort_bits &&
        (rc = hpn_sort_pairs_u64_bits(c, (uint64_t *)u->key.p, (uint32_t *)u->val.p, n, 0, (int)u->sort_bits)) != HPN_OK)
        return rc;
    HPN_HIP(c, launch_bamsort_psize((const uint32_t *)u->size.p, (const uint32_t *)u->val.p, n, (uint32_t *)u->psize.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = hpn_excl_scan(c, n ? u->psize.p : nullptr, 32, u->out_off.p, 64, n)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(&u->payload, (const u64 *)u->out_off.p + n, 8, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (u->payload != u->store_len)
        return fail(c, HPN_E_HIP, "hpn_bam_sort: the sorted records take %llu bytes, the store holds %llu", (unsigned long long)u->payload,
                    (unsigned long long)u->store_len);
    res->payload_bytes = u->payload, res->fresh_mem = u->fresh_mem, res->sort_bits = u->sort_bits;
    return HPN_OK;
}

int hpn_bam_sort_order(hpn_ctx *c, uint32_t *order, uint64_t n)
{
    if (!c || (n && !order)) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_order", true);
    if (!u) return HPN_E_STATE;
    if (n != u->records) return fail(c, HPN_E_ARG, "hpn_bam_sort_order: %llu entries asked for, the session holds %llu records", (unsigned long long)n,
                                     (unsigned long long)u->records);
    if (!n) return HPN_OK;
    HPN_HIP(c, hipSetDevice(c->device));
    HPN_HIP(c, hipMemcpyAsync(order, u->val.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

int hpn_bam_sort_sizes(hpn_ctx *c, uint32_t *sizes, uint64_t n)
{
    if (!c || (n && !sizes)) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_sizes", true);
    if (!u) return HPN_E_STATE;
    if (n != u->records) return fail(c, HPN_E_ARG, "hpn_bam_sort_sizes: %llu entries asked for, the session holds %llu records", (unsigned long long)n,
                                     (unsigned long long)u->records);
    if (!n) return HPN_OK;
    HPN_HIP(c, hipSetDevice(c->device));
    HPN_HIP(c, hipMemcpyAsync(sizes, u->size.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

int hpn_bam_sort_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_emit", true);
    if (!u) return HPN_E_STATE;
    if (u->ended) return fail(c, HPN_E_STATE, "hpn_bam_sort_emit behind the call that ended the file");
    if (first_record != u->emitted)
        return fail(c, HPN_E_ARG, "hpn_bam_sort_emit: slice from record %llu, the next one is %llu (the open block is carried from slice to slice)",
                    (unsigned long long)first_record, (unsigned long long)u->emitted);
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    info->bad_record = -1, info->tid_first = 0, info->tid_last = -1;
    u->list.clear(), u->payload_bytes = 0, u->stored_bytes = 0, u->stored_made = false;
    const uint64_t left = u->records - first_record, cnt = max_records < left ? max_records : left;
    if (cnt > 0xfffffff0ull) return fail(c, HPN_E_ARG, "more than 2^32 records in one slice");
    if (last && cnt != left) return fail(c, HPN_E_ARG, "hpn_bam_sort_emit: last = 1 with %llu records behind the slice", (unsigned long long)(left - cnt));
    info->n_records = cnt;
    const uint64_t m = cnt + 1;
    int rc;
    u64 span[2] = {0, 0};      // the slice's bytes in the sorted payload
    if (cnt) {
        HPN_HIP(c, hipMemcpyAsync(&span[0], (const u64 *)u->out_off.p + first_record, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipMemcpyAsync(&span[1], (const u64 *)u->out_off.p + first_record + cnt, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (span[1] < span[0] || span[1] > u->payload) return fail(c, HPN_E_HIP, "hpn_bam_sort: the slice's offsets are out of order");
    }
    const uint64_t rec_bytes = span[1] - span[0], total = u->fill + rec_bytes;
    if ((rc = scratch_reserve(c, u->Q, (m + 1) * sizeof(u64))) != HPN_OK || (rc = scratch_reserve(c, u->ikey, (m + 1) * sizeof(uint32_t))) != HPN_OK ||
        (rc = cut_reserve(c, u->cw, m)) != HPN_OK || (rc = scratch_reserve(c, u->pay, total + 64)) != HPN_OK)
        return rc;
    const u64 init[4] = {~0ull, 0, 0, 0};
    HPN_HIP(c, hipMemcpyAsync(u->cut_info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    if (u->fill) HPN_HIP(c, hipMemcpyAsync(u->pay.p, u->keep.p, u->fill, hipMemcpyDeviceToDevice, c->stream));
    HPN_HIP(c, launch_bamsort_items((const u64 *)u->out_off.p, first_record, cnt, u->fill, u->fill ? 0u : kCutNoKey, (u64 *)u->Q.p, (uint32_t *)u->ikey.p,
                                    c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_bamsort_gather((const uint8_t *)u->store.p, (const u64 *)u->soff.p, (const uint32_t *)u->size.p, (const uint32_t *)u->val.p,
                                     (const u64 *)u->out_off.p, first_record, cnt, (uint8_t *)u->pay.p + u->fill, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (`init` is this call's)
    if ((rc = cut_blocks(c, u->cw, (const u64 *)u->Q.p, (const uint32_t *)u->ikey.p, m, 1, (u64 *)u->cut_info.p, total, u->list, "hpn_bam_sort")) != HPN_OK)
        return rc;
    int32_t open_tid = -1;
    if ((rc = carry_open(c, u->keep, (const uint8_t *)u->pay.p, u->list, total, last != 0, &u->fill, &open_tid)) != HPN_OK) return rc;
    if (last) u->ended = true;
    if ((rc = close_blocks(c, u->cw, (const uint8_t *)u->pay.p, u->list, false, &u->payload_bytes, &u->stored_bytes)) != HPN_OK) return rc;
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->emitted += cnt;
    info->n_blocks = u->list.size(), info->payload_bytes = u->payload_bytes, info->open_bytes = u->fill;
    if (!u->list.empty()) info->tid_first = info->tid_last = 0;
    return HPN_OK;
}

int hpn_bam_sort_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    if (!c || !n) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_blocks", true);
    if (!u) return HPN_E_STATE;
    const uint64_t have = u->list.size();
    if (first > have) return fail(c, HPN_E_ARG, "block %llu of %llu", (unsigned long long)first, (unsigned long long)have);
    *n = have - first;
    if (*n > cap) return HPN_E_CAPACITY;
    if (*n && !out) return HPN_E_ARG;
    if (*n) memcpy(out, u->list.data() + first, (size_t)*n * sizeof(hpn_split_block));
    return HPN_OK;
}

int hpn_bam_sort_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    if (!c || !d_payload || !n_bytes) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_payload_dev", true);
    if (!u) return HPN_E_STATE;
    *d_payload = (const uint8_t *)u->pay.p, *n_bytes = u->payload_bytes;
    return HPN_OK;
}

// (made when it is asked for: only a level-0 writer wants it)
int hpn_bam_sort_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    if (!c || !d_image || !n_bytes) return HPN_E_ARG;
    hpn_bamsort_state *u = live(c, "hpn_bam_sort_stored_dev", true);
    if (!u) return HPN_E_STATE;
    HPN_HIP(c, hipSetDevice(c->device));
    if (!u->stored_made) {
        const int rc = stored_image(c, u->cw, (const uint8_t *)u->pay.p, u->list, &u->stored_bytes);
        if (rc != HPN_OK) return rc;
        u->stored_made = true;
    }
    *d_image = (const uint8_t *)u->cw.img.p, *n_bytes = u->stored_bytes;
    return HPN_OK;
}

}  // extern "C"
