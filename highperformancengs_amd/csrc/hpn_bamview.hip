// hpn_bamview.hip -- C ABI of samtools' view (sam_view.c, bam.c of samtools-0.1.19): hpn_bam_view_begin / _add_raw_dev / _finish /
// _order, for BAM output _emit / _blocks / _payload_dev / _stored_dev, for text _text_emit / _text_dev.  Kernels:
// kernels/bam_view.hip; the scans through hpn_excl_scan (device pointers); the record store and the BAM slices (gather, cuts,
// CRC-32, stored framing): hpn_bamrec.hpp, whose SliceOut::patch carries -Q's rescaled qualities in front of the CRC-32.
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch: every record's size, keep bit and, for
// text, line length into arrays by ordinal, and the batch's records appended to the record store by one copy.  _finish scans the
// keep bits into order[] and n_out -- the count -- and, for text, the kept lines' lengths into 64-bit offsets.
#include <string.h>

#include <string>
#include <vector>

#include "hpn_bamrec.hpp"
#include "kernels/bam_view.hpp"

using namespace hpn;

struct hpn_view_work : RecSession {      // what a new session must not inherit
    Scratch keep, llen;                  // by ordinal, grown batch by batch
    Scratch kidx, placed, klen, toff, text, names, name_off, ids, id_off;
    VwRules rules = {};
    uint64_t text_bytes = 0, text_emitted = 0, text_n = 0;    // all lines; output records handed out; bytes of the last slice
};

struct hpn_view_state : FamilyState, hpn_view_work {
    static constexpr int kSlot = kStBamView;
    static constexpr const char *kName = "hpn_bam_view", *kVerb = "kept";
    static int wrong_count(hpn_ctx *c, const char *who, uint64_t n, uint64_t want)
    {
        return fail(c, HPN_E_ARG, "%s: %llu entries asked for, the output has %llu records", who, (unsigned long long)n, (unsigned long long)want);
    }
};

namespace {

// SliceOut::patch: the slice lies gathered, the cuts and the CRC-32 come behind this
int scale_slice(hpn_ctx *c, void *arg, const uint32_t *, const u64 *out_off, uint64_t first, uint64_t cnt, uint8_t *pay)
{
    hpn_view_state *u = (hpn_view_state *)arg;
    HPN_HIP(c, launch_bamview_qscale(out_off, first, cnt, u->rules.qual_scale, pay, c->stream));
    return HPN_OK;
}

int bad_of_batch(hpn_ctx *c, hpn_view_state &u, const uint8_t *d_raw, u64 word, uint64_t base)
{
    return bad_from_batch(c, d_raw, word >> kVwReasonBits, base, (uint32_t)(word & ((1u << kVwReasonBits) - 1u)), u.bad);
}

hpn_view_state *live_as(hpn_ctx *c, const char *who, uint32_t emit)
{
    hpn_view_state *u = rec_live<hpn_view_state>(c, who, kRecFinished);
    if (u && u->rules.emit != emit)
        return fail(c, HPN_E_STATE, "%s on a session that emits %s", who, u->rules.emit == kVwBam ? "BAM" : u->rules.emit == kVwText ? "text" : "the count only"),
               nullptr;
    return u;
}

}  // namespace

extern "C" {

int hpn_bam_view_begin(hpn_ctx *c, const hpn_view_opts *o)
{
    if (!c || !o || o->emit > HPN_VIEW_COUNT || o->flag_style > 2u || o->n_targets < 0 || o->threshold > (1u << 24)) return HPN_E_ARG;
    const bool text = o->emit == HPN_VIEW_TEXT;
    if (text && o->n_targets && (!o->target_names || !o->target_name_off)) return HPN_E_ARG;
    if ((o->n_rg_ids && !o->rg_ids) || (o->n_lib_ids && !o->lib_ids) || (o->n_rg_ids && !o->has_rg_ids) || (o->n_lib_ids && !o->has_library)) return HPN_E_ARG;
    // the read-group rule's IDs behind one another: -r's, -R's, the library's
    std::string ids;
    std::vector<uint32_t> id_off(1, 0u);
    auto take = [&](const char *id) { ids += id ? id : "", id_off.push_back((uint32_t)ids.size()); };
    if (o->rg_id) take(o->rg_id);
    for (uint32_t k = 0; k < o->n_rg_ids; ++k) take(o->rg_ids[k]);
    for (uint32_t k = 0; k < o->n_lib_ids; ++k) take(o->lib_ids[k]);
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_view_state *u = state_make<hpn_view_state>(c);
    static_cast<hpn_view_work &>(*u) = hpn_view_work();
    const uint32_t nt = text ? (uint32_t)o->n_targets : 0u;
    const uint32_t name_bytes = nt ? o->target_name_off[nt] : 0u;
    for (uint32_t t = 0; t < nt; ++t)
        if (o->target_name_off[t] > o->target_name_off[t + 1]) return fail(c, HPN_E_ARG, "hpn_bam_view_begin: the targets' name offsets are out of order");
    int rc;
    if ((rc = scratch_reserve(c, u->info, kBsWords * sizeof(u64))) != HPN_OK || (rc = sliceout_begin(c, u->out)) != HPN_OK ||
        (rc = scratch_reserve(c, u->names, (size_t)name_bytes + 4)) != HPN_OK || (rc = scratch_reserve(c, u->name_off, ((size_t)nt + 1) * 4)) != HPN_OK ||
        (rc = scratch_reserve(c, u->ids, ids.size() + 4)) != HPN_OK || (rc = scratch_reserve(c, u->id_off, id_off.size() * 4)) != HPN_OK)
        return rc;
    u64 init[kBsWords] = {0};
    init[kBsBad] = ~0ull;
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    if (name_bytes) HPN_HIP(c, hipMemcpyAsync(u->names.p, o->target_names, name_bytes, hipMemcpyHostToDevice, c->stream));
    if (nt) HPN_HIP(c, hipMemcpyAsync(u->name_off.p, o->target_name_off, ((size_t)nt + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (!ids.empty()) HPN_HIP(c, hipMemcpyAsync(u->ids.p, ids.data(), ids.size(), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemcpyAsync(u->id_off.p, id_off.data(), id_off.size() * 4, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (`init`, the tables and the caller's arrays are free to go)
    const uint32_t rule = (o->rg_id ? kVwRuleId : 0u) | (o->has_rg_ids ? kVwRuleSet : 0u) | (o->has_library ? kVwRuleLib : 0u);
    u->rules = VwRules{o->flag_on, o->flag_off, o->min_mapq, o->min_qlen, o->qual_scale, o->subsample ? 1u : 0u, o->seed, o->threshold, o->emit, o->flag_style,
                       nt, (const uint8_t *)u->names.p, (const uint32_t *)u->name_off.p,
                       rule, o->rg_id ? 1u : 0u, o->n_rg_ids, o->n_lib_ids, (const uint8_t *)u->ids.p, (const uint32_t *)u->id_off.p};
    u->open = true;
    return HPN_OK;
}

int hpn_bam_view_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, hpn_view_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_view_state *u = rec_live<hpn_view_state>(c, "hpn_bam_view_add_raw_dev", kRecFeeding);
    if (!u) return HPN_E_STATE;
    return rec_add(c, *u, d_raw, info, kVwrRecords, {{&u->keep, 4}, {&u->llen, 4}}, [&](uint64_t n, uint64_t base) {
        return launch_bamview_classify(d_raw, (const uint64_t *)c->r_off.p, n, base, u->st.len, u->rules, (uint32_t *)u->st.size.p, (u64 *)u->st.soff.p,
                                       (uint32_t *)u->keep.p, (uint32_t *)u->llen.p, (u64 *)u->info.p, c->stream);
    }, bad_of_batch);
}

int hpn_bam_view_finish(hpn_ctx *c, hpn_view_result *res)
{
    hpn_view_state *u;
    int rc = rec_finish_open(c, "hpn_bam_view_finish", res, u);
    if (!u) return rc;
    const uint64_t n = u->st.records;
    if ((rc = need(c, u->kidx, (n + 1) * 4)) != HPN_OK || (rc = need(c, u->placed, n * 4)) != HPN_OK) return rc;
    if ((rc = hpn_excl_scan(c, n ? u->keep.p : nullptr, 32, u->kidx.p, 32, n)) != HPN_OK) return rc;
    uint32_t n_out = 0;
    HPN_HIP(c, hipMemcpyAsync(&n_out, (const uint32_t *)u->kidx.p + n, 4, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, launch_bamview_compact((const uint32_t *)u->keep.p, (const uint32_t *)u->kidx.p, n, (uint32_t *)u->placed.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->n_out = n_out, u->order = (const uint32_t *)u->placed.p;
    res->n_out = n_out;
    if (u->rules.emit == kVwBam) {
        if (u->rules.qual_scale > 1) u->out.patch = scale_slice, u->out.patch_arg = u;
        if ((rc = sliceout_reserve(c, u->out, n)) != HPN_OK || (rc = sliceout_offsets(c, u->out, u->st, u->order, u->n_out, false, "hpn_bam_view")) != HPN_OK)
            return rc;
        res->payload_bytes = u->out.payload;
    } else if (u->rules.emit == kVwText) {
        // the kept lines' lengths on 64 bits: text outgrows 2^32 long before the store does
        if ((rc = need(c, u->klen, (uint64_t)n_out * 8)) != HPN_OK || (rc = need(c, u->toff, ((uint64_t)n_out + 1) * 8)) != HPN_OK) return rc;
        HPN_HIP(c, launch_bamview_klen((const uint32_t *)u->llen.p, u->order, n_out, (u64 *)u->klen.p, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = hpn_excl_scan(c, n_out ? u->klen.p : nullptr, 64, u->toff.p, 64, n_out)) != HPN_OK) return rc;
        HPN_HIP(c, hipMemcpyAsync(&u->text_bytes, (const u64 *)u->toff.p + n_out, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        res->text_bytes = u->text_bytes;
    }
    return HPN_OK;
}

int hpn_bam_view_order(hpn_ctx *c, uint32_t *order, uint64_t n)
{
    return rec_order<hpn_view_state>(c, "hpn_bam_view_order", order, n);
}

int hpn_bam_view_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_view_state *u = live_as(c, "hpn_bam_view_emit", kVwBam);
    return !u ? HPN_E_STATE : sliceout_emit(c, u->out, u->st, u->order, u->n_out, first_record, max_records, last, info, hpn_view_state::kName);
}

int hpn_bam_view_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    if (!c || !n) return HPN_E_ARG;
    hpn_view_state *u = live_as(c, "hpn_bam_view_blocks", kVwBam);
    return !u ? HPN_E_STATE : list_blocks(c, u->out.list, first, out, cap, n);
}

int hpn_bam_view_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    if (!c || !d_payload || !n_bytes) return HPN_E_ARG;
    hpn_view_state *u = live_as(c, "hpn_bam_view_payload_dev", kVwBam);
    return !u ? HPN_E_STATE : sliceout_payload(u->out, d_payload, n_bytes);
}

int hpn_bam_view_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    if (!c || !d_image || !n_bytes) return HPN_E_ARG;
    hpn_view_state *u = live_as(c, "hpn_bam_view_stored_dev", kVwBam);
    return !u ? HPN_E_STATE : sliceout_stored(c, u->out, d_image, n_bytes);
}

int hpn_bam_view_text_emit(hpn_ctx *c, uint64_t first_record, uint64_t max_records, hpn_view_text_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_view_state *u = live_as(c, "hpn_bam_view_text_emit", kVwText);
    if (!u) return HPN_E_STATE;
    if (first_record != u->text_emitted)
        return fail(c, HPN_E_ARG, "hpn_bam_view_text_emit: slice from record %llu, the next one is %llu", (unsigned long long)first_record,
                    (unsigned long long)u->text_emitted);
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    u->text_n = 0;
    const uint64_t left = u->n_out - first_record, cnt = max_records < left ? max_records : left;
    if (cnt > 0xfffffffull) return fail(c, HPN_E_ARG, "more than 2^28 records in one text slice");
    u64 span[2] = {0, 0};
    if (cnt) {
        HPN_HIP(c, hipMemcpyAsync(&span[0], (const u64 *)u->toff.p + first_record, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipMemcpyAsync(&span[1], (const u64 *)u->toff.p + first_record + cnt, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (span[1] < span[0] || span[1] > u->text_bytes) return fail(c, HPN_E_HIP, "hpn_bam_view: the slice's line offsets are out of order");
    }
    const uint64_t bytes = span[1] - span[0];
    const int rc = scratch_reserve(c, u->text, bytes + 64);
    if (rc != HPN_OK) return rc;
    HPN_HIP(c, launch_bamview_format((const uint8_t *)u->st.store.p, (const u64 *)u->st.soff.p, (const uint32_t *)u->st.size.p, u->order, (const u64 *)u->toff.p,
                                     first_record, cnt, u->rules, (uint8_t *)u->text.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->text_emitted += cnt, u->text_n = bytes;
    info->n_records = cnt, info->n_bytes = bytes;
    return HPN_OK;
}

int hpn_bam_view_text_dev(hpn_ctx *c, const uint8_t **d_text, uint64_t *n_bytes)
{
    if (!c || !d_text || !n_bytes) return HPN_E_ARG;
    hpn_view_state *u = live_as(c, "hpn_bam_view_text_dev", kVwText);
    if (!u) return HPN_E_STATE;
    *d_text = (const uint8_t *)u->text.p, *n_bytes = u->text_n;
    return HPN_OK;
}

}  // extern "C"
