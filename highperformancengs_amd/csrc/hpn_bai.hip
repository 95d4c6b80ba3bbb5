// hpn_bai.hip -- C ABI of samtools' `index`: hpn_bam_bai_begin / _add_raw_dev / _finish / _read.  Kernels: kernels/bam_bai.hip.
//
// The session sees the batches hpn_bam_raw_index_dev has indexed, in file order.  Per batch the device makes the per-record pass
// (checks, counts, linear-index minima) and hands back the batch's run heads -- {start offset, bin, refID} of every record that
// starts a run of equal (refID, stored bin) --, about two per read that straddles a 16 kb boundary.  A chunk runs from its head's offset to the next
// head's, so at the end the lists are made of the heads alone: grouped by (refID, bin) in file order, neighbours joined where
// one ends in the BGZF block the next starts in, the metadata of bin 37450 from where the targets change.  The linear index is
// filled on the device and copied out up to the length its target's last mapped record set.
#include <string.h>

#include <algorithm>
#include <vector>

#include "hpn_bamrec.hpp"

namespace hpn {
// kernels/bam_bai.hip
uint32_t bai_tiles(uint64_t n);
hipError_t launch_bai_records(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, int32_t n_ref, uint64_t base, const void *blk, const u64 *addr,
                              uint32_t nb, const int32_t *target_len, const u64 *win_base, const void *prev, void *next, uint8_t *head, u64 *counts,
                              u64 *last_mapped, u64 *lin, u64 *tile_sum, u64 *info, hipStream_t st);
hipError_t launch_bai_emit(const uint8_t *raw, const uint64_t *rec_off, const uint8_t *head, uint64_t n, const void *blk, const u64 *addr, uint32_t nb,
                           const void *prev, const u64 *tile_base, void *out, uint64_t n_out, hipStream_t st);
hipError_t launch_bai_fill(u64 *lin, const u64 *win_base, const u64 *last_mapped, int32_t n_ref, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
struct Head {            // (kernels/bam_bai.hip writes the same layout)
    uint64_t start;
    uint32_t bin;
    int32_t tid;
};
constexpr uint64_t kMaxWindows = (uint64_t)1 << 27;      // 1 GiB of linear index: more targets x length than any assembly has
constexpr uint64_t kMaxHeads = (uint64_t)1 << 27;        // 2 GiB of run heads on the host (about two per read that straddles a 16 kb boundary: ~10^7 in 10^9 reads of 150 bp)
constexpr size_t kStateBytes = 24;
}  // namespace

struct hpn_bai_state : FamilyState {
    static constexpr int kSlot = kStBai;
    bool open = false, dead = false, ended = false, finished = false;
    int32_t n_ref = 0;
    Scratch tlen, wbase, counts, lastm, lin, state, info, head, tiles, heads, addr;
    int turn = 0;
    uint64_t records = 0, n_no_coor = 0, first_voffset = 0, end_voffset = 0;
    std::vector<uint64_t> h_wbase;
    std::vector<Head> h_heads;             // every run head since _begin, in file order
    BadRecord bad;
    std::vector<hpn_bai_target> targets;
    std::vector<hpn_bai_chunk> chunks;
    std::vector<uint64_t> windows;
};

extern "C" {

int hpn_bam_bai_begin(hpn_ctx *c, int32_t n_ref, const int32_t *target_len, uint64_t first_voffset)
{
    if (!c || n_ref < 0 || (n_ref && !target_len)) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_bai_state *u = state_make<hpn_bai_state>(c);
    u->open = false;
    u->h_wbase.assign((size_t)n_ref + 1, 0);
    for (int32_t t = 0; t < n_ref; ++t)
        u->h_wbase[(size_t)t + 1] = u->h_wbase[(size_t)t] + (target_len[t] > 0 ? (uint64_t)((target_len[t] - 1) >> 14) + 1 : 0);
    const uint64_t total = u->h_wbase[(size_t)n_ref];
    if (total > kMaxWindows) return fail(c, HPN_E_ARG, "hpn_bam_bai_begin: %llu windows of 16 kb in all targets", (unsigned long long)total);
    const size_t nr = (size_t)n_ref;
    int rc;
    if ((rc = scratch_reserve(c, u->tlen, (nr + 1) * sizeof(int32_t))) != HPN_OK || (rc = scratch_reserve(c, u->wbase, (nr + 1) * sizeof(u64))) != HPN_OK ||
        (rc = scratch_reserve(c, u->counts, (2 * nr + 2) * sizeof(u64))) != HPN_OK || (rc = scratch_reserve(c, u->lastm, (nr + 1) * sizeof(u64))) != HPN_OK ||
        (rc = scratch_reserve(c, u->lin, (total + 1) * sizeof(u64))) != HPN_OK || (rc = scratch_reserve(c, u->state, 2 * kStateBytes)) != HPN_OK ||
        (rc = scratch_reserve(c, u->info, 64)) != HPN_OK)
        return rc;
    if (nr) HPN_HIP(c, hipMemcpyAsync(u->tlen.p, target_len, nr * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemcpyAsync(u->wbase.p, u->h_wbase.data(), (nr + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemsetAsync(u->counts.p, 0, (2 * nr + 2) * sizeof(u64), c->stream));
    HPN_HIP(c, hipMemsetAsync(u->lastm.p, 0, (nr + 1) * sizeof(u64), c->stream));
    HPN_HIP(c, hipMemsetAsync(u->lin.p, 0xff, (total + 1) * sizeof(u64), c->stream));
    struct {
        int32_t tid, pos;
        uint32_t bin, have;
        uint64_t last_end;
    } first[2] = {{-1, 0, 0, 0, first_voffset}, {-1, 0, 0, 0, first_voffset}};
    static_assert(sizeof first == 2 * kStateBytes, "the carried state's layout");
    HPN_HIP(c, hipMemcpyAsync(u->state.p, first, sizeof first, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (the sources are the caller's and this frame's)
    u->open = true, u->dead = false, u->ended = false, u->finished = false;
    u->n_ref = n_ref, u->turn = 0, u->records = 0, u->n_no_coor = 0, u->first_voffset = first_voffset, u->end_voffset = first_voffset;
    u->h_heads.clear();
    u->bad = BadRecord();
    u->targets.clear(), u->chunks.clear(), u->windows.clear();
    return HPN_OK;
}

int hpn_bam_bai_add_raw_dev(hpn_ctx *c, const uint8_t *d_raw, const hpn_bgzf_block *d_blocks, uint64_t n_blocks, const uint64_t *block_addr, int last,
                            uint64_t end_voffset, hpn_bai_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_bai_state *u = state<hpn_bai_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_bai_add_raw_dev before hpn_bam_bai_begin");
    if (u->ended) return fail(c, HPN_E_STATE, "hpn_bam_bai_add_raw_dev behind the call that ended the file");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t n = d_raw ? c->r_n : 0;
    info->n_records = n;
    bad_report(u->bad, info);
    if (last) u->ended = true, u->end_voffset = end_voffset;
    if (u->dead || !n) return HPN_OK;
    if (!d_blocks || !block_addr || !n_blocks || n_blocks > 0xfffffff0ull) return fail(c, HPN_E_ARG, "hpn_bam_bai_add_raw_dev: records without their block table");
    if (n > 0xfffffff0ull) return fail(c, HPN_E_ARG, "more than 2^32 records in one batch");
    const uint32_t tiles = bai_tiles(n);
    int rc;
    if ((rc = scratch_reserve(c, u->head, n + 64)) != HPN_OK || (rc = scratch_reserve(c, u->tiles, ((size_t)tiles + 1) * sizeof(u64))) != HPN_OK ||
        (rc = scratch_reserve(c, u->addr, (n_blocks + 1) * sizeof(u64))) != HPN_OK)
        return rc;
    const u64 init[4] = {~0ull, 0, 0, 0};
    HPN_HIP(c, hipMemcpyAsync(u->info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, hipMemcpyAsync(u->addr.p, block_addr, (n_blocks + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    uint8_t *states = (uint8_t *)u->state.p;
    const void *prev = states + kStateBytes * u->turn;
    HPN_HIP(c, launch_bai_records(d_raw, (const uint64_t *)c->r_off.p, n, u->n_ref, u->records, d_blocks, (const u64 *)u->addr.p, (uint32_t)n_blocks,
                                  (const int32_t *)u->tlen.p, (const u64 *)u->wbase.p, prev, states + kStateBytes * (u->turn ^ 1), (uint8_t *)u->head.p,
                                  (u64 *)u->counts.p, (u64 *)u->lastm.p, (u64 *)u->lin.p, (u64 *)u->tiles.p, (u64 *)u->info.p, c->stream));
    u64 h[4];
    HPN_HIP(c, hipMemcpyAsync(h, u->info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (also: `init` and block_addr are the caller's)
    if (h[0] != ~0ull) {                               // the first record outside the domain: refID and pos for the report
        if ((rc = bad_from_batch(c, d_raw, h[0] >> 4, u->records, (uint32_t)(h[0] & 15), u->bad)) != HPN_OK) return rc;
        u->dead = true;
        u->records += n;
        bad_report(u->bad, info);
        return HPN_OK;
    }
    const uint64_t nh = h[2];
    if (nh > n) return fail(c, HPN_E_HIP, "hpn_bam_bai: %llu run heads in %llu records", (unsigned long long)nh, (unsigned long long)n);
    if (u->h_heads.size() + nh > kMaxHeads) {          // the lists are made on the host: what they may take there is bounded
        u->dead = true;
        u->bad = BadRecord{(int64_t)u->records, 0, 0, 9};
        u->records += n;
        std::vector<Head>().swap(u->h_heads);
        bad_report(u->bad, info);
        return HPN_OK;
    }
    if (nh) {
        if ((rc = scratch_reserve(c, u->heads, nh * sizeof(Head))) != HPN_OK) return rc;
        HPN_HIP(c, launch_bai_emit(d_raw, (const uint64_t *)c->r_off.p, (const uint8_t *)u->head.p, n, d_blocks, (const u64 *)u->addr.p, (uint32_t)n_blocks,
                                   prev, (const u64 *)u->tiles.p, u->heads.p, nh, c->stream));
        const size_t at = u->h_heads.size();
        u->h_heads.resize(at + nh);
        HPN_HIP(c, hipMemcpyAsync(u->h_heads.data() + at, u->heads.p, nh * sizeof(Head), hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
    }
    u->turn ^= 1;
    u->records += n, u->n_no_coor += h[1];
    info->n_runs = nh;
    return HPN_OK;
}

int hpn_bam_bai_finish(hpn_ctx *c, hpn_bai_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_bai_state *u = state<hpn_bai_state>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "hpn_bam_bai_finish before hpn_bam_bai_begin");
    if (!u->dead && !u->ended) return fail(c, HPN_E_STATE, "hpn_bam_bai_finish before the file's end: the last hpn_bam_bai_add_raw_dev takes last = 1");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->n_records = u->records, res->n_no_coor = u->n_no_coor, res->n_ref = (uint32_t)u->n_ref;
    bad_report(u->bad, res);
    u->targets.assign((size_t)u->n_ref, hpn_bai_target{});
    u->chunks.clear(), u->windows.clear();
    u->open = false, u->finished = true;
    if (u->dead || !u->n_ref) return HPN_OK;
    const size_t nr = (size_t)u->n_ref;
    const uint64_t total = u->h_wbase[nr];
    HPN_HIP(c, launch_bai_fill((u64 *)u->lin.p, (const u64 *)u->wbase.p, (const u64 *)u->lastm.p, u->n_ref, c->stream));
    std::vector<u64> counts(2 * nr), lastm(nr), lin((size_t)total);
    HPN_HIP(c, hipMemcpyAsync(counts.data(), u->counts.p, 2 * nr * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipMemcpyAsync(lastm.data(), u->lastm.p, nr * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (total) HPN_HIP(c, hipMemcpyAsync(lin.data(), u->lin.p, (size_t)total * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    // chunks: head j to head j + 1 (the first record without a refID closes the last target's; else the file's end does)
    const std::vector<Head> &H = u->h_heads;
    std::vector<hpn_bai_chunk> all;
    all.reserve(H.size());
    for (size_t j = 0; j < H.size(); ++j) {
        if (H[j].tid < 0) break;
        all.push_back(hpn_bai_chunk{H[j].start, j + 1 < H.size() ? H[j + 1].start : u->end_voffset, H[j].bin, H[j].tid});
    }
    // the metadata: a target's offsets run from where the target before it ended (the first: behind the header) to its own end
    uint64_t off_beg = u->first_voffset;
    for (size_t j = 0; j < all.size();) {
        size_t e = j;
        while (e < all.size() && all[e].tid == all[j].tid) ++e;
        hpn_bai_target &t = u->targets[(size_t)all[j].tid];
        t.has_records = 1, t.off_beg = off_beg, t.off_end = all[e - 1].end;
        t.n_mapped = counts[2 * (size_t)all[j].tid], t.n_unmapped = counts[2 * (size_t)all[j].tid + 1];
        off_beg = t.off_end;
        j = e;
    }
    std::stable_sort(all.begin(), all.end(), [](const hpn_bai_chunk &a, const hpn_bai_chunk &b) { return a.tid != b.tid ? a.tid < b.tid : a.bin < b.bin; });
    for (size_t j = 0; j < all.size(); ++j) {
        const bool joins = !u->chunks.empty() && u->chunks.back().tid == all[j].tid && u->chunks.back().bin == all[j].bin &&
                           u->chunks.back().end >> 16 == all[j].beg >> 16;
        if (joins) u->chunks.back().end = all[j].end;
        else u->chunks.push_back(all[j]);
    }
    for (size_t j = 0; j < u->chunks.size(); ++j) {
        hpn_bai_target &t = u->targets[(size_t)u->chunks[j].tid];
        if (!t.n_chunks) t.first_chunk = j;
        ++t.n_chunks;
    }
    for (size_t t = 0; t < nr; ++t) {
        uint64_t n = lastm[t] & 0xfffffu;
        const uint64_t width = u->h_wbase[t + 1] - u->h_wbase[t];
        if (n > width) n = width;
        u->targets[t].first_window = u->windows.size(), u->targets[t].n_windows = (int32_t)n;
        u->windows.insert(u->windows.end(), lin.begin() + (size_t)u->h_wbase[t], lin.begin() + (size_t)(u->h_wbase[t] + n));
    }
    res->n_chunks = u->chunks.size(), res->n_windows = u->windows.size();
    return HPN_OK;
}

int hpn_bam_bai_read(hpn_ctx *c, hpn_bai_target *targets, hpn_bai_chunk *chunks, uint64_t *windows)
{
    if (!c) return HPN_E_ARG;
    hpn_bai_state *u = state<hpn_bai_state>(c);
    if (!u || !u->finished) return fail(c, HPN_E_STATE, "hpn_bam_bai_read before hpn_bam_bai_finish");
    if ((!u->targets.empty() && !targets) || (!u->chunks.empty() && !chunks) || (!u->windows.empty() && !windows)) return HPN_E_ARG;
    if (!u->targets.empty()) memcpy(targets, u->targets.data(), u->targets.size() * sizeof(hpn_bai_target));
    if (!u->chunks.empty()) memcpy(chunks, u->chunks.data(), u->chunks.size() * sizeof(hpn_bai_chunk));
    if (!u->windows.empty()) memcpy(windows, u->windows.data(), u->windows.size() * sizeof(uint64_t));
    return HPN_OK;
}

}  // extern "C"
