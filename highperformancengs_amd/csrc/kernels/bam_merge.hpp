// bam_merge.hpp -- what kernels/bam_merge.hip and the session over it (hpn_bammerge.hip) share: the info words behind
// bam_sort.hpp's, the tile of the running maximum, the launchers.
#pragma once
#include "bam_sort.hpp"

namespace hpn {

// info words [0..6] and [8] as bam_sort.hpp names them (k_merge_keys fills what k_sort_keys fills, launch_bamsort_rank reads
// them); [7] is not used here;   [9] records whose effective key is not their own (k_merge_apply)
enum { kBmLifted = 9 };

constexpr int kBmThreads = 256, kBmPerThread = 8, kBmTile = kBmThreads * kBmPerThread;      // the running maximum's tile: 2,048 records

inline uint64_t bammerge_tiles(uint64_t n) { return (n + kBmTile - 1) / kBmTile; }

// keys, ordinals, sizes, places and the file number of the batch's n records (ordinals base ..), with the domain check
hipError_t launch_bammerge_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, uint32_t file, u64 *key,
                                uint32_t *val, uint32_t *fid, uint32_t *size, u64 *soff, u64 *info, hipStream_t st);
// key[i] <- the largest key of records [start of i's file, i]; info[kBmLifted] += the records this changed.  tile_fid / tile_key:
// bammerge_tiles(n) entries each.
hipError_t launch_bammerge_runmax(u64 *key, const uint32_t *fid, uint64_t n, uint32_t *tile_fid, u64 *tile_key, u64 *info, hipStream_t st);

}  // namespace hpn
