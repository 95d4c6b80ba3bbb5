// hpn_cuts.hpp -- samtools' writer rule as one launch sequence, shared by the sessions that write BAM: hpn_split.hip (a target's
// records as they lie in the input) and, through hpn_bamrec.hpp's SliceOut, hpn_bamsort.hip and hpn_rmdup.hip (stored records in
// the order the family decided, slice by slice).  Kernels: kernels/bam_split.hip.
//
// A caller describes its payload buffer as m items -- item 0 the bytes of the block the call before left open, items 1 .. m - 1
// its records -- by Q[0 .. m] (where an item starts, Q[m] the end) and key[0 .. m - 1] (the item's target; items of a key outside
// [0, n_ref) make no block).  cut_blocks() lists the blocks bam_write1 would close, carry_open() takes the last one back while
// it may still grow, close_blocks() gives the others their CRC-32 and, for level 0, their stored image.
#pragma once
#include <string.h>

#include <vector>

#include "hpn_ctx.hpp"

namespace hpn {
// kernels/bam_split.hip
uint32_t split_tiles(uint64_t m);
hipError_t launch_split_cuts(const u64 *Q, const uint32_t *key, uint64_t m, int32_t n_ref, uint32_t *a, uint32_t *b, uint32_t *c, uint32_t *mark,
                             u64 *tile_sum, u64 *info, hipStream_t st);
hipError_t launch_split_emit(const u64 *Q, const uint32_t *key, const uint32_t *next, const uint32_t *mark, uint64_t m, int32_t n_ref,
                             const u64 *tile_base, void *out, uint64_t n_out, hipStream_t st);
hipError_t launch_split_stored(const uint8_t *pay, const void *specs, uint32_t n, uint8_t *img, hipStream_t st);

constexpr uint32_t kCutFull = 0xff00;
constexpr uint32_t kCutNoKey = 0xfffffffeu;
typedef hpn_stored_span StoredSpec;      // (kernels/bam_split.hip reads the same layout)

struct CutWork {
    Scratch ja, jb, jc, mark, tiles, blocks, specs, img;
};

inline int cut_reserve(hpn_ctx *c, CutWork &w, uint64_t m)
{
    int rc;
    if ((rc = scratch_reserve(c, w.ja, (m + 1) * sizeof(uint32_t))) != HPN_OK || (rc = scratch_reserve(c, w.jb, (m + 1) * sizeof(uint32_t))) != HPN_OK ||
        (rc = scratch_reserve(c, w.jc, (m + 1) * sizeof(uint32_t))) != HPN_OK || (rc = scratch_reserve(c, w.mark, (m + 1) * sizeof(uint32_t))) != HPN_OK ||
        (rc = scratch_reserve(c, w.tiles, ((size_t)split_tiles(m) + 1) * sizeof(u64))) != HPN_OK)
        return rc;
    return HPN_OK;
}

// The blocks of the m items in file order (off / len inside the payload buffer of `total` bytes; crc not yet set).  info: four
// device words, [3] takes the count.  cut_reserve(m) has been called.
inline int cut_blocks(hpn_ctx *c, CutWork &w, const u64 *Q, const uint32_t *key, uint64_t m, int32_t n_ref, u64 *info, uint64_t total,
                      std::vector<hpn_split_block> &list, const char *who)
{
    int rc;
    HPN_HIP(c, launch_split_cuts(Q, key, m, n_ref, (uint32_t *)w.ja.p, (uint32_t *)w.jb.p, (uint32_t *)w.jc.p, (uint32_t *)w.mark.p, (u64 *)w.tiles.p, info,
                                 c->stream));
    u64 nb = 0;
    HPN_HIP(c, hipMemcpyAsync(&nb, info + 3, sizeof nb, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (nb > total / 32 + 2) return fail(c, HPN_E_HIP, "%s: %llu blocks out of %llu bytes", who, (unsigned long long)nb, (unsigned long long)total);
    list.resize(nb);
    if (nb) {
        if ((rc = scratch_reserve(c, w.blocks, nb * sizeof(hpn_split_block))) != HPN_OK) return rc;
        HPN_HIP(c, launch_split_emit(Q, key, (const uint32_t *)w.ja.p, (const uint32_t *)w.mark.p, m, n_ref, (const u64 *)w.tiles.p, w.blocks.p, nb, c->stream));
        HPN_HIP(c, hipMemcpyAsync(list.data(), w.blocks.p, nb * sizeof(hpn_split_block), hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
    }
    for (const hpn_split_block &b : list)          // (what the host copies by must lie inside the payload)
        if (b.len == 0 || b.len > kCutFull || b.off > total || b.len > total - b.off)
            return fail(c, HPN_E_HIP, "%s: a block of %u bytes at %llu of %llu", who, b.len, (unsigned long long)b.off, (unsigned long long)total);
    return HPN_OK;
}

// The last block stays open while its target may go on: its bytes move into `keep` (0xff00 bytes at least), it leaves the list.
inline int carry_open(hpn_ctx *c, Scratch &keep, const uint8_t *pay, std::vector<hpn_split_block> &list, uint64_t total, bool last, uint32_t *fill,
                      int32_t *open_tid)
{
    *fill = 0, *open_tid = -1;
    if (!last && !list.empty()) {
        const hpn_split_block &b = list.back();
        if (b.off + b.len == total && b.len < kCutFull) {
            HPN_HIP(c, hipMemcpyAsync(keep.p, pay + b.off, b.len, hipMemcpyDeviceToDevice, c->stream));
            *fill = b.len, *open_tid = b.tid;
            list.pop_back();
        }
    }
    return HPN_OK;
}

// The listed blocks (their CRC-32 set) framed as stored BGZF blocks in w.img, one after the other; *stored_bytes: the image's size.
inline int stored_image(hpn_ctx *c, CutWork &w, const uint8_t *pay, const std::vector<hpn_split_block> &list, uint64_t *stored_bytes)
{
    *stored_bytes = 0;
    const size_t nc = list.size();
    if (!nc) return HPN_OK;
    int rc;
    std::vector<StoredSpec> specs(nc);
    uint64_t at = 0;
    for (size_t k = 0; k < nc; ++k) {
        specs[k] = StoredSpec{list[k].off, at, list[k].len, list[k].crc};
        at += (uint64_t)list[k].len + 31;
    }
    if ((rc = scratch_reserve(c, w.specs, nc * sizeof(StoredSpec))) != HPN_OK || (rc = scratch_reserve(c, w.img, at + 64)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(w.specs.p, specs.data(), nc * sizeof(StoredSpec), hipMemcpyHostToDevice, c->stream));
    HPN_HIP(c, launch_split_stored(pay, w.specs.p, (uint32_t)nc, (uint8_t *)w.img.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));      // (`specs` is this call's)
    *stored_bytes = at;
    return HPN_OK;
}

// CRC-32 of every listed block; with level0 their stored image as well.  *payload_bytes: the bytes of the payload buffer the
// blocks cover.
inline int close_blocks(hpn_ctx *c, CutWork &w, const uint8_t *pay, std::vector<hpn_split_block> &list, bool level0, uint64_t *payload_bytes,
                        uint64_t *stored_bytes)
{
    *payload_bytes = 0, *stored_bytes = 0;
    const size_t nc = list.size();
    if (!nc) return HPN_OK;
    int rc;
    std::vector<hpn_span> spans(nc);
    std::vector<uint32_t> crcs(nc);
    for (size_t k = 0; k < nc; ++k) spans[k] = hpn_span{list[k].off, list[k].len};
    if ((rc = hpn_crc32_dev(c, pay, spans.data(), (uint32_t)nc, crcs.data())) != HPN_OK) return rc;
    for (size_t k = 0; k < nc; ++k) list[k].crc = crcs[k];
    *payload_bytes = list.back().off + list.back().len;
    return level0 ? stored_image(c, w, pay, list, stored_bytes) : (int)HPN_OK;
}

// The listed blocks from `first` on into out[0 .. cap): what a family's _blocks call answers.
inline int list_blocks(hpn_ctx *c, const std::vector<hpn_split_block> &list, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    const uint64_t have = list.size();
    if (first > have) return fail(c, HPN_E_ARG, "block %llu of %llu", (unsigned long long)first, (unsigned long long)have);
    *n = have - first;
    if (*n > cap) return HPN_E_CAPACITY;
    if (*n && !out) return HPN_E_ARG;
    if (*n) memcpy(out, list.data() + first, (size_t)*n * sizeof(hpn_split_block));
    return HPN_OK;
}

}  // namespace hpn
