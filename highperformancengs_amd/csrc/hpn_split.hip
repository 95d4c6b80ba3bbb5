// hpn_split.hip -- C ABI of bamSplitChr.c: hpn_bam_split_begin / _add_raw_dev / _blocks / _payload_dev / _stored_dev / _finish.
// Kernels: kernels/bam_split.hip; the CRC-32 of the closed blocks through hpn_crc32_dev (kernels/crc32.hip).
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch: keys and checks, the batch's
// records copied behind the bytes of the block the batch before left open (the payload buffer), the cuts, the block list, the
// CRCs, for level 0 the stored image; the last block stays open unless it is full, its target has ended or the file has.
#include <string.h>

#include <vector>

#include "hpn_bamrec.hpp"

namespace hpn {
// kernels/bam_split.hip (the cuts, the block list and the stored framing: hpn_cuts.hpp)
hipError_t launch_split_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, int32_t n_ref, uint64_t base, uint32_t fill,
                             uint32_t open_key, const void *prev, void *next, u64 *Q, uint32_t *key, u64 *counts, u64 *info, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
constexpr uint32_t kFull = kCutFull;
constexpr uint32_t kNoKey = kCutNoKey;
}  // namespace

struct hpn_split_state : FamilyState {
    static constexpr int kSlot = kStSplit;
    bool open = false, dead = false, ended = false;
    int32_t n_ref = 0;
    bool level0 = false;
    Scratch Q, key, pay, keep, counts, state, info;
    CutWork cw;
    int turn = 0;                    // which of the two carried states the next batch reads
    uint64_t records = 0, n_blocks = 0;
    uint32_t fill = 0;               // bytes of the open block (in `keep`)
    int32_t open_tid = -1;
    BadRecord bad;
    std::vector<hpn_split_block> list;   // the closed blocks of the last call
    uint64_t payload_bytes = 0, stored_bytes = 0;
};

extern "C" {

int hpn_bam_split_begin(hpn_ctx *c, int32_t n_ref, int level0)
{
    if (!c || n_ref < 0) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_split_state *u = state_make<hpn_split_state>(c);
    int rc;
    if ((rc = scratch_reserve(c, u->counts, ((size_t)n_ref + 1) * sizeof(u64))) != HPN_OK) return rc;
    if ((rc = scratch_reserve(c, u->state, 64)) != HPN_OK || (rc = scratch_reserve(c, u->info, 64)) != HPN_OK) return rc;
    if ((rc = scratch_reserve(c, u->keep, kFull + 64)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemsetAsync(u->counts.p, 0, ((size_t)n_ref + 1) * sizeof(u64), c->stream));
    HPN_HIP(c, hipMemsetAsync(u->state.p, 0, 64, c->stream));
    u->open = true, u->dead = false, u->ended = false;
    u->n_ref = n_ref, u->level0 = level0 != 0;
    u->turn = 0, u->records = 0, u->n_blocks = 0, u->fill = 0, u->open_tid = -1;
    u->bad = BadRecord();
    u->list.clear(), u->payload_bytes = 0, u->stored_bytes = 0;
    return HPN_OK;
}

static void split_report(const hpn_split_state *u, hpn_split_info *info)
{
    bad_report(u->bad, info);
    info->tid_first = 0, info->tid_last = -1;
}

int hpn_bam_split_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, int last, hpn_split_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_split_state *u = state<hpn_split_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_split_add_raw_dev before hpn_bam_split_begin");
    if (u->ended) return fail(c, HPN_E_STATE, "hpn_bam_split_add_raw_dev behind the call that ended the file");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    u->list.clear(), u->payload_bytes = 0, u->stored_bytes = 0;
    const uint64_t n = d_raw ? c->r_n : 0;
    info->n_records = n;
    split_report(u, info);
    if (u->dead) return HPN_OK;                        // outside the domain: nothing more is made
    if (n > 0xfffffff0ull) return fail(c, HPN_E_ARG, "more than 2^32 records in one batch");
    const uint64_t m = n + 1;
    int rc;
    if ((rc = scratch_reserve(c, u->Q, (m + 1) * sizeof(u64))) != HPN_OK || (rc = scratch_reserve(c, u->key, (m + 1) * sizeof(uint32_t))) != HPN_OK ||
        (rc = cut_reserve(c, u->cw, m)) != HPN_OK)
        return rc;
    const u64 init[4] = {~0ull, 0, 0, 0};
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    uint8_t *states = (uint8_t *)u->state.p;
    HPN_HIP(c, launch_split_keys(d_raw, (const uint64_t *)c->r_off.p, n, u->n_ref, u->records, u->fill, u->fill ? (uint32_t)u->open_tid : kNoKey,
                                 states + 16 * u->turn, states + 16 * (u->turn ^ 1), (u64 *)u->Q.p, (uint32_t *)u->key.p, (u64 *)u->counts.p,
                                 (u64 *)u->info.p, c->stream));
    u64 h[4];
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (also: `init` is the caller's stack)
    u->turn ^= 1;
    if (h[0] != ~0ull) {                               // the first record outside the domain: refID and pos for the message
        if ((rc = bad_from_batch(c, d_raw, h[0] >> 3, u->records, (uint32_t)(h[0] & 7), u->bad)) != HPN_OK) return rc;
        u->dead = true;
        u->records += n;
        split_report(u, info);
        return HPN_OK;
    }
    u->records += n;
    // the payload: the open block's bytes, then the batch's records as they lie in the stream
    const uint64_t rec_bytes = n ? h[2] - h[1] : 0, total = u->fill + rec_bytes;
    if ((rc = scratch_reserve(c, u->pay, total + 64)) != HPN_OK) return rc;
    if (u->fill) HPN_HIP(c, hipMemcpyAsync(u->pay.p, u->keep.p, u->fill, hipMemcpyDeviceToDevice, c->stream));
    if (rec_bytes) HPN_HIP(c, hipMemcpyAsync((uint8_t *)u->pay.p + u->fill, d_raw + h[1], rec_bytes, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = cut_blocks(c, u->cw, (const u64 *)u->Q.p, (const uint32_t *)u->key.p, m, u->n_ref, (u64 *)u->info.p, total, u->list, "hpn_bam_split")) != HPN_OK) return rc;
    // the last block stays open while its target may go on
    if ((rc = carry_open(c, u->keep, (const uint8_t *)u->pay.p, u->list, total, last != 0, &u->fill, &u->open_tid)) != HPN_OK) return rc;
    if (last) u->ended = true;
    const size_t nc = u->list.size();
    if ((rc = close_blocks(c, u->cw, (const uint8_t *)u->pay.p, u->list, u->level0, &u->payload_bytes, &u->stored_bytes)) != HPN_OK) return rc;
    if (nc) info->tid_first = u->list.front().tid, info->tid_last = u->list.back().tid;
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->n_blocks += nc;
    info->n_blocks = nc, info->payload_bytes = u->payload_bytes, info->stored_bytes = u->stored_bytes, info->open_bytes = u->fill;
    return HPN_OK;
}

int hpn_bgzf_stored_dev(hpn_ctx *c, const uint8_t *d_data, const hpn_stored_span *spans, uint32_t n_spans, uint8_t *d_image)
{
    if (!c || (n_spans && (!d_data || !spans || !d_image))) return HPN_E_ARG;
    for (uint32_t k = 0; k < n_spans; ++k)
        if (spans[k].len == 0 || spans[k].len > kFull) return fail(c, HPN_E_ARG, "hpn_bgzf_stored_dev: span %u has %u bytes", k, spans[k].len);
    if (!n_spans) return HPN_OK;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_split_state *u = state_make<hpn_split_state>(c);
    const int rc = scratch_reserve(c, u->cw.specs, (size_t)n_spans * sizeof(StoredSpec));
    if (rc != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(u->cw.specs.p, spans, (size_t)n_spans * sizeof(StoredSpec), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, launch_split_stored(d_data, u->cw.specs.p, n_spans, d_image, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

int hpn_bam_split_blocks(hpn_ctx *c, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    if (!c || !n) return HPN_E_ARG;
    hpn_split_state *u = state<hpn_split_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_split_blocks before hpn_bam_split_begin");
    return list_blocks(c, u->list, first, out, cap, n);
}

int hpn_bam_split_payload_dev(hpn_ctx *c, const uint8_t **d_payload, uint64_t *n_bytes)
{
    if (!c || !d_payload || !n_bytes) return HPN_E_ARG;
    hpn_split_state *u = state<hpn_split_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_split_payload_dev before hpn_bam_split_begin");
    *d_payload = (const uint8_t *)u->pay.p, *n_bytes = u->payload_bytes;
    return HPN_OK;
}

int hpn_bam_split_stored_dev(hpn_ctx *c, const uint8_t **d_image, uint64_t *n_bytes)
{
    if (!c || !d_image || !n_bytes) return HPN_E_ARG;
    hpn_split_state *u = state<hpn_split_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_split_stored_dev before hpn_bam_split_begin");
    if (!u->level0) return fail(c, HPN_E_STATE, "hpn_bam_split_stored_dev: the session was not begun with level0");
    *d_image = (const uint8_t *)u->cw.img.p, *n_bytes = u->stored_bytes;
    return HPN_OK;
}

int hpn_bam_split_finish(hpn_ctx *c, hpn_split_result *res, uint64_t *counts)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_split_state *u = state<hpn_split_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_split_finish before hpn_bam_split_begin");
    if (!u->dead && u->fill) return fail(c, HPN_E_STATE, "hpn_bam_split_finish with a block open: the last hpn_bam_split_add_raw_dev takes last = 1");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->n_records = u->records, res->n_blocks = u->n_blocks, res->n_ref = (uint32_t)u->n_ref;
    bad_report(u->bad, res);
    if (counts && u->n_ref) {
        // (per batch the counts moved by ordinals INSIDE the batch: every batch adds its own records, the sums are the file's)
        HPN_HIP(c, hipMemcpyAsync(counts, u->counts.p, (size_t)u->n_ref * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
    }
    u->open = false;
    return HPN_OK;
}

}  // extern "C"
