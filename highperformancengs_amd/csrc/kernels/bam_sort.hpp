// bam_sort.hpp -- what kernels/bam_sort.hip and the sessions over it (hpn_bamsort.hip; hpn_bamrec.hpp for hpn_rmdup.hip as well)
// share: the info words, the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpn {
typedef unsigned long long u64;

// info (u64 words, kept on the device from _begin to _finish):
//   [0] lowest (ordinal << 3 | reason), ~0 none      [1] stream offset of the batch's first record   [2] ... behind its last
//   [3] smallest high word below 2^31 (~0 none)       [4] largest such + 1 (0 none)
//   [5] smallest high word from 2^31 up (~0 none)     [6] largest such - 0x7fffffff (0 none)
//   [7] sum of 72 + kroundup32(block_size - 32)       [8] largest remapped key (k_sort_rank)
enum { kBsBad = 0, kBsFirst, kBsEnd, kBsLoMin, kBsLoMax, kBsHiMin, kBsHiMax, kBsMem, kBsMaxKey, kBsWords = 16 };

hipError_t launch_bamsort_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, u64 *key, uint32_t *val,
                               uint32_t *size, u64 *soff, u64 *info, hipStream_t st);
hipError_t launch_bamsort_rank(u64 *key, uint64_t n, u64 *info, hipStream_t st);
hipError_t launch_bamsort_psize(const uint32_t *size, const uint32_t *order, uint64_t n, uint32_t *psize, hipStream_t st);
// psize[j] = size[order[j]] + extra[order[j]]: a family whose records grow on their way out (hpn_bamrec.hpp: SliceOut::extra)
hipError_t launch_bamsort_psize_grown(const uint32_t *size, const uint32_t *extra, const uint32_t *order, uint64_t n, uint32_t *psize, hipStream_t st);
hipError_t launch_bamsort_items(const u64 *out_off, uint64_t first, uint64_t cnt, uint32_t fill, uint32_t open_key, u64 *Q, uint32_t *key, hipStream_t st);
hipError_t launch_bamsort_gather(const uint8_t *store, const u64 *soff, const uint32_t *size, const uint32_t *order, const u64 *out_off, uint64_t first,
                                 uint64_t cnt, uint8_t *pay, int n_cu, hipStream_t st);

// bits [0, bits_of(v)) hold v: the range a radix sort over keys up to v runs over
inline int bits_of(uint64_t v)
{
    int b = 0;
    for (; v; v >>= 1) ++b;
    return b;
}

}  // namespace hpn
