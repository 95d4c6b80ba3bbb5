// hpn_rmdup.hip -- C ABI of samtools' rmdup of a coordinate-sorted BAM (bam_rmdup.c, pairs): hpn_bam_rmdup_begin / _add_raw_dev /
// _finish / _counts / _order / _emit / _blocks / _payload_dev / _stored_dev.  Kernels: kernels/bam_rmdup.hip; the gather, the
// sizes and the items of a slice: kernels/bam_sort.hip; the radix sort and the scan through hpn_sort_pairs_u64_bits and
// hpn_excl_scan (device pointers); the record store and the slices (gather, cuts, CRC-32, stored framing): hpn_bamrec.hpp.
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch: every record's fields, class, name
// hash, quality sum and library into arrays by ordinal -- the left neighbour of a batch's first record is the entry the batch
// before wrote, so a batch may end anywhere --, and the batch's records appended to the record store by one copy.  _finish works
// on the arrays alone: runs, groups, name events, placement (the order of the kernels is the order of kernels/bam_rmdup.hip's
// header).  _emit is hpn_bam_sort_emit's: the next slice of the surviving records gathered behind the open block and cut.
#include <string.h>

#include <vector>

#include "hpn_bamrec.hpp"
#include "kernels/bam_rmdup.hpp"

using namespace hpn;

namespace {
constexpr uint32_t kMaxIds = 1u << 16;
}  // namespace

struct hpn_rmdup_work : RecSession {   // what a new session must not inherit
    Scratch tp, cls, isize, qsum, lib, hash;                                                     // by ordinal, grown batch by batch
    Scratch rb, hf, rsc, hsc, rid, runstart, evkind, evrec, slot, drop, now, sl, cnow, cslot;    // _finish
    Scratch hkey, hval, ekey, eval, placed;                                                      // (placed: the output's order)
    Scratch id_bytes, id_off, id_lib, libs, unmatched, present;
    uint32_t n_ref = 0, n_ids = 0, n_libs = 0;
    uint64_t n_heads = 0;
};

struct hpn_rmdup_state : FamilyState, hpn_rmdup_work {
    static constexpr int kSlot = kStBamRmdup;
    static constexpr const char *kName = "hpn_bam_rmdup", *kVerb = "decided";
    static int wrong_count(hpn_ctx *c, const char *who, uint64_t n, uint64_t want)
    {
        return fail(c, HPN_E_ARG, "%s: %llu entries asked for, %llu records survive", who, (unsigned long long)n, (unsigned long long)want);
    }
};

static_assert(kRmBad == kInfoBad && kRmFirst == kInfoFirst && kRmEnd == kInfoEnd, "k_rm_classify's info words are the sessions'");

namespace {

RmArrays arrays_of(hpn_rmdup_state *u)
{
    return RmArrays{(u64 *)u->tp.p, (uint32_t *)u->cls.p, (uint32_t *)u->isize.p, (uint32_t *)u->qsum.p, (uint32_t *)u->lib.p, (uint32_t *)u->st.size.p,
                    (u64 *)u->hash.p, (u64 *)u->st.soff.p};
}

// The record the device names, by both of rmdup's kernels that check -- k_rm_classify per batch, k_rm_names in _finish --:
// 4 reason bits, and its refID and pos for the caller's message from tp[], which holds them by ordinal (rec_add's bad_of).
int note_bad(hpn_ctx *c, hpn_rmdup_state &u, const uint8_t *, u64 word, uint64_t)
{
    const uint64_t ord = word >> 4;
    u64 tp = 0;
    HPN_HIP(c, hipMemcpyAsync(&tp, (const u64 *)u.tp.p + ord, sizeof tp, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u.bad.record = (int64_t)ord, u.bad.tid = (int32_t)(tp >> 32), u.bad.pos = (int32_t)(uint32_t)tp, u.bad.reason = (uint32_t)(word & 15);
    return HPN_OK;
}

}  // namespace

extern "C" {

int hpn_bam_rmdup_begin(hpn_ctx *c, int32_t n_ref, uint32_t n_ids, const char *const *ids, const uint32_t *lib_of_id, uint32_t n_libs)
{
    if (!c || n_ref < 0 || n_libs < 1 || (n_ids && (!ids || !lib_of_id))) return HPN_E_ARG;
    if (n_ids > kMaxIds) return fail(c, HPN_E_ARG, "hpn_bam_rmdup_begin: %u IDs, the table takes %u", n_ids, kMaxIds);
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off(1, 0u), lib;
    for (uint32_t k = 0; k < n_ids; ++k) {
        if (!ids[k] || lib_of_id[k] >= n_libs) return fail(c, HPN_E_ARG, "hpn_bam_rmdup_begin: ID %u has no name or a library beyond %u", k, n_libs);
        bytes.insert(bytes.end(), (const uint8_t *)ids[k], (const uint8_t *)ids[k] + strlen(ids[k]));
        off.push_back((uint32_t)bytes.size()), lib.push_back(lib_of_id[k]);
    }
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_rmdup_state *u = state_make<hpn_rmdup_state>(c);
    static_cast<hpn_rmdup_work &>(*u) = hpn_rmdup_work();
    u->n_ref = (uint32_t)n_ref, u->n_ids = n_ids, u->n_libs = n_libs;
    int rc;
    if ((rc = scratch_reserve(c, u->info, kRmWords * sizeof(u64))) != HPN_OK || (rc = sliceout_begin(c, u->out)) != HPN_OK ||
        (rc = scratch_reserve(c, u->id_bytes, bytes.size() + 64)) != HPN_OK ||
        (rc = scratch_reserve(c, u->id_off, off.size() * 4)) != HPN_OK || (rc = scratch_reserve(c, u->id_lib, (lib.size() + 1) * 4)) != HPN_OK ||
        (rc = scratch_reserve(c, u->libs, (size_t)n_libs * 3 * sizeof(u64))) != HPN_OK ||
        (rc = scratch_reserve(c, u->unmatched, ((size_t)n_ref + 1) * sizeof(u64))) != HPN_OK ||
        (rc = scratch_reserve(c, u->present, ((size_t)n_ref + 1) * sizeof(uint32_t))) != HPN_OK)
        return rc;
    u64 init[kRmWords] = {0};
    init[kRmBad] = ~0ull;
    std::vector<u64> libs((size_t)n_libs * 3, 0ull);
    for (uint32_t l = 0; l < n_libs; ++l) libs[3 * (size_t)l + 2] = ~0ull;
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemcpyAsync(u->libs.p, libs.data(), libs.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemsetAsync(u->unmatched.p, 0, ((size_t)n_ref + 1) * sizeof(u64), c->stream));
    HPN_HIP(c, hipMemsetAsync(u->present.p, 0, ((size_t)n_ref + 1) * sizeof(uint32_t), c->stream));
    if (!bytes.empty()) HPN_HIP(c, hipMemcpyAsync(u->id_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemcpyAsync(u->id_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!lib.empty()) HPN_HIP(c, hipMemcpyAsync(u->id_lib.p, lib.data(), lib.size() * 4, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (the host vectors are this call's)
    u->open = true;
    return HPN_OK;
}

int hpn_bam_rmdup_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, hpn_rmdup_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_rmdup_state *u = rec_live<hpn_rmdup_state>(c, "hpn_bam_rmdup_add_raw_dev", kRecFeeding);
    if (!u) return HPN_E_STATE;
    return rec_add(c, *u, d_raw, info, kRsRecords, {{&u->tp, 8}, {&u->cls, 4}, {&u->isize, 4}, {&u->qsum, 4}, {&u->lib, 4}, {&u->hash, 8}},
                   [&](uint64_t n, uint64_t base) {
        const RmIds ids = {(const uint8_t *)u->id_bytes.p, (const uint32_t *)u->id_off.p, (const uint32_t *)u->id_lib.p, u->n_ids};
        return launch_rmdup_classify(d_raw, (const uint64_t *)c->r_off.p, n, base, u->st.len, u->n_ref, arrays_of(u), ids, (u64 *)u->info.p, c->stream);
    }, note_bad);
}

int hpn_bam_rmdup_finish(hpn_ctx *c, hpn_rmdup_result *res)
{
    hpn_rmdup_state *u;
    int rc = rec_finish_open(c, "hpn_bam_rmdup_finish", res, u, [](hpn_rmdup_state &s, hpn_rmdup_result *r) { r->n_libs = s.n_libs, r->n_ref = s.n_ref; });
    if (!u) return rc;
    auto report = [&]() {
        res->n_out = u->n_out, res->payload_bytes = u->out.payload, res->n_heads = u->n_heads;
        bad_report(u->bad, res);
    };
    const uint64_t n = u->st.records;
    Scratch *per_record[] = {&u->rb, &u->hf, &u->rid, &u->evkind, &u->evrec, &u->slot, &u->drop, &u->now, &u->sl, &u->hval, &u->eval, &u->placed};
    for (Scratch *s : per_record)
        if ((rc = need(c, *s, n * 4)) != HPN_OK) return rc;
    Scratch *scanned[] = {&u->rsc, &u->hsc, &u->cnow, &u->cslot, &u->runstart};
    for (Scratch *s : scanned)
        if ((rc = need(c, *s, (n + 2) * 4)) != HPN_OK) return rc;
    if ((rc = need(c, u->hkey, n * 8)) != HPN_OK || (rc = need(c, u->ekey, n * 8)) != HPN_OK || (rc = sliceout_reserve(c, u->out, n)) != HPN_OK) return rc;
    const RmArrays A = arrays_of(u);
    const RmWork W = {(uint32_t *)u->rb.p,     (uint32_t *)u->hf.p,    (uint32_t *)u->rsc.p,  (uint32_t *)u->hsc.p,  (uint32_t *)u->rid.p,
                      (uint32_t *)u->runstart.p, (uint32_t *)u->evkind.p, (uint32_t *)u->evrec.p, (uint32_t *)u->slot.p, (uint32_t *)u->drop.p,
                      (uint32_t *)u->now.p,    (uint32_t *)u->sl.p,    (uint32_t *)u->cnow.p, (uint32_t *)u->cslot.p};
    u64 *hkey = (u64 *)u->hkey.p, *ekey = (u64 *)u->ekey.p;
    uint32_t *hval = (uint32_t *)u->hval.p, *eval = (uint32_t *)u->eval.p, *order = (uint32_t *)u->placed.p;
    uint32_t counts[2] = {0, 0};      // runs, heads
    if (n) {
        // runs and heads
        HPN_HIP(c, launch_rmdup_runs(A, W, n, u->n_ref, (uint32_t *)u->present.p, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = hpn_excl_scan(c, W.rb, 32, W.rsc, 32, n)) != HPN_OK || (rc = hpn_excl_scan(c, W.hf, 32, W.hsc, 32, n)) != HPN_OK) return rc;
        HPN_HIP(c, hipMemcpyAsync(&counts[0], W.rsc + n, 4, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipMemcpyAsync(&counts[1], W.hsc + n, 4, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, launch_rmdup_scatter(A, W, n, hkey, hval, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        const uint64_t n_runs = counts[0], m = counts[1];
        if (n_runs < 1 || n_runs > n || m > n) return fail(c, HPN_E_HIP, "hpn_bam_rmdup: %llu runs and %llu heads of %llu records", (unsigned long long)n_runs,
                                                          (unsigned long long)m, (unsigned long long)n);
        u->n_heads = m;
        // groups: the heads by (run, library, isize), in their order inside a group
        if (m > 1 && (rc = hpn_sort_pairs_u64_bits(c, (uint64_t *)hkey, hval, m, 0, 32 + bits_of(u->n_libs - 1))) != HPN_OK) return rc;
        HPN_HIP(c, launch_rmdup_runkey(W, m, hkey, hval, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (m > 1 && bits_of(n_runs - 1) && (rc = hpn_sort_pairs_u64_bits(c, (uint64_t *)hkey, hval, m, 0, bits_of(n_runs - 1))) != HPN_OK) return rc;
        HPN_HIP(c, launch_rmdup_groups(A, W, m, hval, (u64 *)u->libs.p, c->stream));
        // names: the events in time order, sorted by the name's hash
        HPN_HIP(c, launch_rmdup_evkey(A, W, n, ekey, eval, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (n > 1 && (rc = hpn_sort_pairs_u64_bits(c, (uint64_t *)ekey, eval, n, 0, 64)) != HPN_OK) return rc;
        HPN_HIP(c, launch_rmdup_names((const uint8_t *)u->st.store.p, A, W, n, ekey, eval, (u64 *)u->unmatched.p, (u64 *)u->info.p, c->stream));
        u64 bad = ~0ull;
        HPN_HIP(c, hipMemcpyAsync(&bad, u->info.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (bad != ~0ull) {
            if ((rc = note_bad(c, *u, nullptr, bad, 0)) != HPN_OK) return rc;
            u->dead = true;
            report();
            return HPN_OK;
        }
        // placement
        HPN_HIP(c, launch_rmdup_flags(A, W, n, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = hpn_excl_scan(c, W.now, 32, W.cnow, 32, n)) != HPN_OK || (rc = hpn_excl_scan(c, W.sl, 32, W.cslot, 32, n)) != HPN_OK) return rc;
        uint32_t kept[2] = {0, 0};
        HPN_HIP(c, hipMemcpyAsync(&kept[0], W.cnow + n, 4, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipMemcpyAsync(&kept[1], W.cslot + n, 4, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->n_out = (uint64_t)kept[0] + kept[1];
        if (u->n_out > n) return fail(c, HPN_E_HIP, "hpn_bam_rmdup: %llu records out of %llu", (unsigned long long)u->n_out, (unsigned long long)n);
        HPN_HIP(c, hipMemsetAsync(order, 0, n * 4, c->stream));          // (every entry is written below; an ordinal in any case)
        HPN_HIP(c, launch_rmdup_place(W, n, u->n_out, order, c->stream));
    }
    u->order = order;
    if ((rc = sliceout_offsets(c, u->out, u->st, order, u->n_out, false, "hpn_bam_rmdup")) != HPN_OK) return rc;
    report();
    return HPN_OK;
}

int hpn_bam_rmdup_counts(hpn_ctx *c, hpn_rmdup_lib *libs, hpn_rmdup_target *targets)
{
    if (!c || !libs || !targets) return HPN_E_ARG;
    hpn_rmdup_state *u = rec_live<hpn_rmdup_state>(c, "hpn_bam_rmdup_counts", kRecFinished);
    if (!u) return HPN_E_STATE;
    HPN_HIP(c, hipSetDevice(c->device));
    const size_t nt = (size_t)u->n_ref + 1;
    std::vector<u64> w((size_t)u->n_libs * 3), un(nt);
    std::vector<uint32_t> pr(nt);
    HPN_HIP(c, hipMemcpyAsync(w.data(), u->libs.p, w.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipMemcpyAsync(un.data(), u->unmatched.p, nt * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipMemcpyAsync(pr.data(), u->present.p, nt * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < nt; ++t) targets[t].unmatched = un[t], targets[t].has_records = pr[t], targets[t].reserved = 0;
    for (uint32_t l = 0; l < u->n_libs; ++l)
        libs[l].checked = w[3 * (size_t)l], libs[l].removed = w[3 * (size_t)l + 1], libs[l].first = w[3 * (size_t)l + 2] == ~0ull ? -1 : (int64_t)w[3 * (size_t)l + 2];
    return HPN_OK;
}

int hpn_bam_rmdup_order(hpn_ctx *c, uint32_t *order, uint64_t n)
{
    return rec_order<hpn_rmdup_state>(c, "hpn_bam_rmdup_order", order, n);
}

int hpn_bam_rmdup_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    return rec_emit<hpn_rmdup_state>(c, "hpn_bam_rmdup_emit", first_record, max_records, last, info);
}

int hpn_bam_rmdup_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    return rec_blocks<hpn_rmdup_state>(c, "hpn_bam_rmdup_blocks", first, out, cap, n);
}

int hpn_bam_rmdup_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    return rec_payload<hpn_rmdup_state>(c, "hpn_bam_rmdup_payload_dev", d_payload, n_bytes);
}

int hpn_bam_rmdup_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    return rec_stored<hpn_rmdup_state>(c, "hpn_bam_rmdup_stored_dev", d_image, n_bytes);
}

}  // extern "C"
