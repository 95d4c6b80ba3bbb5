// hpn_bamfixmate.hip -- C ABI of samtools' fixmate (bam_mate.c, samtools-0.1.19): hpn_bam_fixmate_begin / _add_raw_dev / _finish /
// _order / _emit / _blocks / _payload_dev / _stored_dev.  Kernels: kernels/bam_fixmate.hip; the scan through hpn_excl_scan (device
// pointers); the record store and the slices (gather, cuts, CRC-32, stored framing): hpn_bamrec.hpp, whose SliceOut lets the
// records grow (`extra`) and be rewritten between the gather and the cuts (`patch`).
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch: every record's size, class, alignment
// end, updated flag and CIGAR text length into arrays by ordinal, and the batch's records appended to the record store by one
// copy.  _finish works on the arrays and reads names and core fields from the store, so a pair whose halves lie in two batches is
// like any other: live records numbered, names compared with the live record in front, runs numbered, roles, write counts, their
// scan, order[] and the patches.  _emit gathers a slice, patches it and cuts it.
#include <string.h>

#include <vector>

#include "hpn_bamrec.hpp"
#include "kernels/bam_fixmate.hpp"

using namespace hpn;

struct hpn_fixmate_work : RecSession {   // what a new session must not inherit
    Scratch meta, cend, clen;                                                     // by ordinal, grown batch by batch
    Scratch live, lidx, liveidx, head, rid, runstart, role, writes, woff, placed;  // _finish (placed: the output's order)
    Scratch pflag, pmtid, pmpos, pisize, extra, partner;
    Scratch target_len;
    int remove_reads = 0;
    uint32_t n_targets = 0;
};

struct hpn_fixmate_state : FamilyState, hpn_fixmate_work {
    static constexpr int kSlot = kStBamFixmate;
    static constexpr const char *kName = "hpn_bam_fixmate", *kVerb = "fixed";
    static int wrong_count(hpn_ctx *c, const char *who, uint64_t n, uint64_t want)
    {
        return fail(c, HPN_E_ARG, "%s: %llu entries asked for, the output has %llu records", who, (unsigned long long)n, (unsigned long long)want);
    }
};

namespace {

FxRecords records_of(hpn_fixmate_state *u)
{
    return FxRecords{(const uint8_t *)u->st.store.p, (const u64 *)u->st.soff.p, (const uint32_t *)u->st.size.p, (uint32_t *)u->meta.p, (int32_t *)u->cend.p,
                     (uint32_t *)u->clen.p};
}

FxPatch patch_of(hpn_fixmate_state *u)
{
    return FxPatch{(uint32_t *)u->pflag.p, (uint32_t *)u->pmtid.p, (uint32_t *)u->pmpos.p, (uint32_t *)u->pisize.p, (uint32_t *)u->extra.p,
                   (uint32_t *)u->partner.p};
}

// SliceOut::patch: the slice lies gathered, the cuts and the CRC-32 come behind this
int patch_slice(hpn_ctx *c, void *arg, const uint32_t *order, const u64 *out_off, uint64_t first, uint64_t cnt, uint8_t *pay)
{
    hpn_fixmate_state *u = (hpn_fixmate_state *)arg;
    HPN_HIP(c, launch_bamfix_apply(records_of(u), patch_of(u), order, out_off, first, cnt, pay, c->stream));
    return HPN_OK;
}

}  // namespace

extern "C" {

int hpn_bam_fixmate_begin(hpn_ctx *c, int remove_reads, int32_t n_targets, const uint32_t *target_len)
{
    if (!c || n_targets < 0 || (n_targets && !target_len)) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_fixmate_state *u = state_make<hpn_fixmate_state>(c);
    static_cast<hpn_fixmate_work &>(*u) = hpn_fixmate_work();
    u->remove_reads = remove_reads ? 1 : 0, u->n_targets = (uint32_t)n_targets;
    int rc;
    if ((rc = scratch_reserve(c, u->info, kBsWords * sizeof(u64))) != HPN_OK || (rc = sliceout_begin(c, u->out)) != HPN_OK ||
        (rc = scratch_reserve(c, u->target_len, ((size_t)n_targets + 1) * 4)) != HPN_OK)
        return rc;
    u64 init[kBsWords] = {0};
    init[kBsBad] = ~0ull;
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    if (n_targets) HPN_HIP(c, hipMemcpyAsync(u->target_len.p, target_len, (size_t)n_targets * 4, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (`init` and the caller's array are free to go)
    u->open = true;
    return HPN_OK;
}

int hpn_bam_fixmate_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, hpn_fixmate_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_fixmate_state *u = rec_live<hpn_fixmate_state>(c, "hpn_bam_fixmate_add_raw_dev", kRecFeeding);
    if (!u) return HPN_E_STATE;
    return rec_add(c, *u, d_raw, info, kFxrRecords, {{&u->meta, 4}, {&u->cend, 4}, {&u->clen, 4}}, [&](uint64_t n, uint64_t base) {
        return launch_bamfix_classify(d_raw, (const uint64_t *)c->r_off.p, n, base, u->st.len, u->n_targets, (const uint32_t *)u->target_len.p,
                                      (uint32_t *)u->st.size.p, (u64 *)u->st.soff.p, (uint32_t *)u->meta.p, (int32_t *)u->cend.p, (uint32_t *)u->clen.p,
                                      (u64 *)u->info.p, c->stream);
    }, rec_bad_of_batch<hpn_fixmate_state>);
}

int hpn_bam_fixmate_finish(hpn_ctx *c, hpn_fixmate_result *res)
{
    hpn_fixmate_state *u;
    int rc = rec_finish_open(c, "hpn_bam_fixmate_finish", res, u);
    if (!u) return rc;
    const uint64_t n = u->st.records;
    if ((rc = sliceout_reserve(c, u->out, n)) != HPN_OK || (rc = need(c, u->live, n * 4)) != HPN_OK || (rc = need(c, u->lidx, (n + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->role, n * 4)) != HPN_OK || (rc = need(c, u->writes, n * 4)) != HPN_OK || (rc = need(c, u->woff, (n + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->placed, n * 4)) != HPN_OK || (rc = need(c, u->pflag, n * 4)) != HPN_OK || (rc = need(c, u->pmtid, n * 4)) != HPN_OK ||
        (rc = need(c, u->pmpos, n * 4)) != HPN_OK || (rc = need(c, u->pisize, n * 4)) != HPN_OK || (rc = need(c, u->extra, n * 4)) != HPN_OK ||
        (rc = need(c, u->partner, n * 4)) != HPN_OK)
        return rc;
    const FxRecords r = records_of(u);
    // the live records: numbered, listed
    HPN_HIP(c, launch_bamfix_live(r.meta, n, (uint32_t *)u->live.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = hpn_excl_scan(c, n ? u->live.p : nullptr, 32, u->lidx.p, 32, n)) != HPN_OK) return rc;
    uint32_t n_live = 0;
    HPN_HIP(c, hipMemcpyAsync(&n_live, (const uint32_t *)u->lidx.p + n, 4, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = need(c, u->liveidx, (uint64_t)n_live * 4)) != HPN_OK || (rc = need(c, u->head, (uint64_t)n_live * 4)) != HPN_OK ||
        (rc = need(c, u->rid, ((uint64_t)n_live + 1) * 4)) != HPN_OK || (rc = need(c, u->runstart, (uint64_t)n_live * 4)) != HPN_OK)
        return rc;
    HPN_HIP(c, launch_bamfix_compact(r.meta, (const uint32_t *)u->lidx.p, n, (uint32_t *)u->liveidx.p, c->stream));
    // runs of equal names among them, and every run's start
    HPN_HIP(c, launch_bamfix_heads(r, (const uint32_t *)u->liveidx.p, n_live, (uint32_t *)u->head.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = hpn_excl_scan(c, n_live ? u->head.p : nullptr, 32, u->rid.p, 32, n_live)) != HPN_OK) return rc;
    HPN_HIP(c, launch_bamfix_runstart((const uint32_t *)u->head.p, (const uint32_t *)u->rid.p, n_live, (uint32_t *)u->runstart.p, c->stream));
    // roles, what every record makes the reference write, and from the scan of that the order
    HPN_HIP(c, launch_bamfix_roles(r.meta, (const uint32_t *)u->lidx.p, n, n_live, (const uint32_t *)u->head.p, (const uint32_t *)u->rid.p,
                                   (const uint32_t *)u->runstart.p, u->remove_reads, (uint32_t *)u->role.p, (uint32_t *)u->writes.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = hpn_excl_scan(c, n ? u->writes.p : nullptr, 32, u->woff.p, 32, n)) != HPN_OK) return rc;
    HPN_HIP(c, launch_bamfix_plan(r, (const uint32_t *)u->lidx.p, (const uint32_t *)u->liveidx.p, n, (const uint32_t *)u->role.p,
                                  (const uint32_t *)u->writes.p, (const uint32_t *)u->woff.p, (uint32_t *)u->placed.p, patch_of(u), (u64 *)u->info.p, c->stream));
    u64 h[kBsWords];
    uint32_t triggered = 0, last_role = kFxSkipped, last_live = 0;
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipMemcpyAsync(&triggered, (const uint32_t *)u->woff.p + n, 4, hipMemcpyDeviceToHost, c->stream));
    if (n_live) HPN_HIP(c, hipMemcpyAsync(&last_live, (const uint32_t *)u->liveidx.p + (n_live - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (n_live) {
        HPN_HIP(c, hipMemcpyAsync(&last_role, (const uint32_t *)u->role.p + last_live, 4, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
    }
    u->n_out = (uint64_t)triggered + (last_role == kFxPending ? 1u : 0u);      // the pending record at the end of the file is written last
    u->order = (const uint32_t *)u->placed.p;
    u->out.extra = (const uint32_t *)u->extra.p, u->out.grown = h[kFxAdded];
    u->out.patch = patch_slice, u->out.patch_arg = u;
    if ((rc = sliceout_offsets(c, u->out, u->st, u->order, u->n_out, !u->remove_reads, "hpn_bam_fixmate")) != HPN_OK) return rc;
    res->n_out = u->n_out, res->n_pairs = h[kFxPairs], res->n_singletons = h[kFxSingles], res->n_tags = h[kFxTags], res->bytes_added = h[kFxAdded];
    res->payload_bytes = u->out.payload;
    return HPN_OK;
}

int hpn_bam_fixmate_order(hpn_ctx *c, uint32_t *order, uint64_t n)
{
    return rec_order<hpn_fixmate_state>(c, "hpn_bam_fixmate_order", order, n);
}

int hpn_bam_fixmate_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    return rec_emit<hpn_fixmate_state>(c, "hpn_bam_fixmate_emit", first_record, max_records, last, info);
}

int hpn_bam_fixmate_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    return rec_blocks<hpn_fixmate_state>(c, "hpn_bam_fixmate_blocks", first, out, cap, n);
}

int hpn_bam_fixmate_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    return rec_payload<hpn_fixmate_state>(c, "hpn_bam_fixmate_payload_dev", d_payload, n_bytes);
}

int hpn_bam_fixmate_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    return rec_stored<hpn_fixmate_state>(c, "hpn_bam_fixmate_stored_dev", d_image, n_bytes);
}

}  // extern "C"
