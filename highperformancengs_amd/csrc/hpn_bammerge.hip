// hpn_bammerge.hip -- C ABI of samtools' merge (bam_sort.c: bam_merge_core2): hpn_bam_merge_begin / _next_file / _add_raw_dev /
// _finish / _order / _emit / _blocks / _payload_dev / _stored_dev.  Kernels: kernels/bam_merge.hip, and kernels/bam_sort.hip's
// rank of the high words; the radix sort and the scan through hpn_sort_pairs_u64_bits and hpn_excl_scan (device pointers); the
// record store and the slices (gather, cuts, CRC-32, stored framing): hpn_bamrec.hpp, over hpn_cuts.hpp.
//
// The session sees the input files in argument order and, inside a file, the batches hpn_bam_raw_index_dev has indexed, in file
// order.  Per batch: the heap's keys, sizes, the file number and the check for the one key the heap cannot hold, and the batch's
// records appended to the record store by one copy -- so the store is file-major.  _finish ranks the high words, replaces every key
// by the largest one of its own file up to it, and sorts (key, ordinal) stably over the bits the keys use: equal keys keep the
// store's order, file before file, which is the heap's tie rule.  _emit hands the output back slice by slice as hpn_bam_sort_emit
// does.
#include <string.h>

#include <vector>

#include "hpn_bamrec.hpp"
#include "kernels/bam_merge.hpp"

using namespace hpn;

struct hpn_bammerge_work : RecSession {   // what a new session must not inherit
    Scratch key, val, fid, tile_fid, tile_key;
    uint64_t n_files = 0;
    uint32_t sort_bits = 0;
};

struct hpn_bammerge_state : FamilyState, hpn_bammerge_work {
    static constexpr int kSlot = kStBamMerge;
    static constexpr const char *kName = "hpn_bam_merge", *kVerb = "merged";
    static int wrong_count(hpn_ctx *c, const char *who, uint64_t n, uint64_t want)
    {
        return fail(c, HPN_E_ARG, "%s: %llu entries asked for, the session holds %llu records", who, (unsigned long long)n, (unsigned long long)want);
    }
};

extern "C" {

int hpn_bam_merge_begin(hpn_ctx *c)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_bammerge_state *u = state_make<hpn_bammerge_state>(c);
    static_cast<hpn_bammerge_work &>(*u) = hpn_bammerge_work();
    int rc;
    if ((rc = scratch_reserve(c, u->info, kBsWords * sizeof(u64))) != HPN_OK || (rc = sliceout_begin(c, u->out)) != HPN_OK) return rc;
    u64 init[kBsWords] = {0};
    init[kBsBad] = init[kBsLoMin] = init[kBsHiMin] = ~0ull;
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (`init` is this call's)
    u->open = true;
    return HPN_OK;
}

int hpn_bam_merge_next_file(hpn_ctx *c)
{
    if (!c) return HPN_E_ARG;
    hpn_bammerge_state *u = rec_live<hpn_bammerge_state>(c, "hpn_bam_merge_next_file", kRecFeeding);
    if (!u) return HPN_E_STATE;
    if (u->n_files >= 0xffffffffull) return fail(c, HPN_E_ARG, "hpn_bam_merge_next_file: more than 2^32 - 1 files");
    ++u->n_files;
    return HPN_OK;
}

int hpn_bam_merge_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, hpn_bammerge_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_bammerge_state *u = rec_live<hpn_bammerge_state>(c, "hpn_bam_merge_add_raw_dev", kRecFeeding);
    if (!u) return HPN_E_STATE;
    if (!u->n_files) return fail(c, HPN_E_STATE, "hpn_bam_merge_add_raw_dev before the first hpn_bam_merge_next_file");
    // (a bad record here is the first one with the HEAP_EMPTY key)
    return rec_add(c, *u, d_raw, info, kBmrRecords, {{&u->key, 8}, {&u->val, 4}, {&u->fid, 4}}, [&](uint64_t n, uint64_t base) {
        return launch_bammerge_keys(d_raw, (const uint64_t *)c->r_off.p, n, base, u->st.len, (uint32_t)(u->n_files - 1), (u64 *)u->key.p, (uint32_t *)u->val.p,
                                    (uint32_t *)u->fid.p, (uint32_t *)u->st.size.p, (u64 *)u->st.soff.p, (u64 *)u->info.p, c->stream);
    }, rec_bad_of_batch<hpn_bammerge_state>);
}

int hpn_bam_merge_finish(hpn_ctx *c, hpn_bammerge_result *res)
{
    hpn_bammerge_state *u;
    int rc = rec_finish_open(c, "hpn_bam_merge_finish", res, u, [](hpn_bammerge_state &s, hpn_bammerge_result *r) { r->n_files = s.n_files; });
    if (!u) return rc;
    const uint64_t n = u->st.records, tiles = bammerge_tiles(n);
    u->order = (const uint32_t *)u->val.p, u->n_out = n;         // (val: the ordinals, sorted in place below)
    if ((rc = sliceout_reserve(c, u->out, n)) != HPN_OK || (rc = need(c, u->tile_fid, (tiles + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->tile_key, (tiles + 1) * 8)) != HPN_OK)
        return rc;
    // the ranks keep the keys' order, so the largest key of a file's front is the same record before and behind the remap
    HPN_HIP(c, launch_bamsort_rank((u64 *)u->key.p, n, (u64 *)u->info.p, c->stream));
    HPN_HIP(c, launch_bammerge_runmax((u64 *)u->key.p, (const uint32_t *)u->fid.p, n, (uint32_t *)u->tile_fid.p, (u64 *)u->tile_key.p, (u64 *)u->info.p,
                                      c->stream));
    u64 h[kBsWords];
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->sort_bits = (uint32_t)bits_of(h[kBsMaxKey]);    // bit 0 up to the highest bit set in any key (the effective keys have the same maximum)
    if (n > 1 && u->sort_bits &&
        (rc = hpn_sort_pairs_u64_bits(c, (uint64_t *)u->key.p, (uint32_t *)u->val.p, n, 0, (int)u->sort_bits)) != HPN_OK)
        return rc;
    if ((rc = sliceout_offsets(c, u->out, u->st, u->order, n, true, "hpn_bam_merge")) != HPN_OK) return rc;
    res->payload_bytes = u->out.payload, res->n_lifted = h[kBmLifted], res->sort_bits = u->sort_bits;
    return HPN_OK;
}

int hpn_bam_merge_order(hpn_ctx *c, uint32_t *order, uint64_t n)
{
    return rec_order<hpn_bammerge_state>(c, "hpn_bam_merge_order", order, n);
}

int hpn_bam_merge_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    return rec_emit<hpn_bammerge_state>(c, "hpn_bam_merge_emit", first_record, max_records, last, info);
}

int hpn_bam_merge_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    return rec_blocks<hpn_bammerge_state>(c, "hpn_bam_merge_blocks", first, out, cap, n);
}

int hpn_bam_merge_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    return rec_payload<hpn_bammerge_state>(c, "hpn_bam_merge_payload_dev", d_payload, n_bytes);
}

int hpn_bam_merge_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    return rec_stored<hpn_bammerge_state>(c, "hpn_bam_merge_stored_dev", d_image, n_bytes);
}

}  // extern "C"
