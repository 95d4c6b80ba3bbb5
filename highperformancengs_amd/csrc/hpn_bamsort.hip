// hpn_bamsort.hip -- C ABI of samtools' coordinate sort (bam_sort.c): hpn_bam_sort_begin / _add_raw_dev / _finish / _order / _sizes /
// _emit / _blocks / _payload_dev / _stored_dev.  Kernels: kernels/bam_sort.hip; the radix sort and the scan through
// hpn_sort_pairs_u64_bits and hpn_excl_scan (device pointers); the record store and the slices (gather, cuts, CRC-32, stored
// framing): hpn_bamrec.hpp, over hpn_cuts.hpp.
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch: keys, sizes and checks, and the
// batch's records -- one slice of the inflated stream -- appended to the record store by one copy.  _finish ranks the high words,
// sorts (key, ordinal) over the bits the keys use, and scans the sorted sizes into output offsets.  _emit gathers the next slice of
// the sorted records behind the bytes of the block the slice before left open, cuts it as bam_write1 would, and keeps the last
// block open for the next slice.
#include <string.h>

#include <vector>

#include "hpn_bamrec.hpp"

using namespace hpn;

struct hpn_bamsort_work : RecSession {   // what a new session must not inherit
    Scratch key, val;
    uint32_t sort_bits = 0;
    uint64_t fresh_mem = 0;
};

struct hpn_bamsort_state : FamilyState, hpn_bamsort_work {
    static constexpr int kSlot = kStBamSort;
    static constexpr const char *kName = "hpn_bam_sort", *kVerb = "sorted";
    static int wrong_count(hpn_ctx *c, const char *who, uint64_t n, uint64_t want)
    {
        return fail(c, HPN_E_ARG, "%s: %llu entries asked for, the session holds %llu records", who, (unsigned long long)n, (unsigned long long)want);
    }
};

extern "C" {

int hpn_bam_sort_begin(hpn_ctx *c)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_bamsort_state *u = state_make<hpn_bamsort_state>(c);
    static_cast<hpn_bamsort_work &>(*u) = hpn_bamsort_work();
    int rc;
    if ((rc = scratch_reserve(c, u->info, kBsWords * sizeof(u64))) != HPN_OK || (rc = sliceout_begin(c, u->out)) != HPN_OK) return rc;
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
    hpn_bamsort_state *u = rec_live<hpn_bamsort_state>(c, "hpn_bam_sort_add_raw_dev", kRecFeeding);
    if (!u) return HPN_E_STATE;
    return rec_add(c, *u, d_raw, info, kBsrRecords, {{&u->key, 8}, {&u->val, 4}}, [&](uint64_t n, uint64_t base) {
        return launch_bamsort_keys(d_raw, (const uint64_t *)c->r_off.p, n, base, u->st.len, (u64 *)u->key.p, (uint32_t *)u->val.p, (uint32_t *)u->st.size.p,
                                   (u64 *)u->st.soff.p, (u64 *)u->info.p, c->stream);
    }, rec_bad_of_batch<hpn_bamsort_state>);
}

int hpn_bam_sort_finish(hpn_ctx *c, hpn_bamsort_result *res)
{
    hpn_bamsort_state *u;
    int rc = rec_finish_open(c, "hpn_bam_sort_finish", res, u);
    if (!u) return rc;
    const uint64_t n = u->st.records;
    u->order = (const uint32_t *)u->val.p, u->n_out = n;         // (val: the ordinals, sorted in place below)
    if ((rc = sliceout_reserve(c, u->out, n)) != HPN_OK) return rc;
    HPN_HIP(c, launch_bamsort_rank((u64 *)u->key.p, n, (u64 *)u->info.p, c->stream));
    u64 h[kBsWords];
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->fresh_mem = h[kBsMem];
    u->sort_bits = (uint32_t)bits_of(h[kBsMaxKey]);    // bit 0 up to the highest bit set in any key
    if (n > 1 && u->sort_bits &&
        (rc = hpn_sort_pairs_u64_bits(c, (uint64_t *)u->key.p, (uint32_t *)u->val.p, n, 0, (int)u->sort_bits)) != HPN_OK)
        return rc;
    if ((rc = sliceout_offsets(c, u->out, u->st, u->order, n, true, "hpn_bam_sort")) != HPN_OK) return rc;
    res->payload_bytes = u->out.payload, res->fresh_mem = u->fresh_mem, res->sort_bits = u->sort_bits;
    return HPN_OK;
}

int hpn_bam_sort_order(hpn_ctx *c, uint32_t *order, uint64_t n)
{
    return rec_order<hpn_bamsort_state>(c, "hpn_bam_sort_order", order, n);
}

int hpn_bam_sort_sizes(hpn_ctx *c, uint32_t *sizes, uint64_t n)
{
    if (!c || (n && !sizes)) return HPN_E_ARG;
    hpn_bamsort_state *u = rec_live<hpn_bamsort_state>(c, "hpn_bam_sort_sizes", kRecFinished);
    if (!u) return HPN_E_STATE;
    return n != u->st.records ? u->wrong_count(c, "hpn_bam_sort_sizes", n, u->st.records) : rec_copy_out(c, sizes, u->st.size.p, n);
}

int hpn_bam_sort_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    return rec_emit<hpn_bamsort_state>(c, "hpn_bam_sort_emit", first_record, max_records, last, info);
}

int hpn_bam_sort_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    return rec_blocks<hpn_bamsort_state>(c, "hpn_bam_sort_blocks", first, out, cap, n);
}

int hpn_bam_sort_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    return rec_payload<hpn_bamsort_state>(c, "hpn_bam_sort_payload_dev", d_payload, n_bytes);
}

int hpn_bam_sort_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    return rec_stored<hpn_bamsort_state>(c, "hpn_bam_sort_stored_dev", d_image, n_bytes);
}

}  // extern "C"
