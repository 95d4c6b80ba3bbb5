// rqc_key.hpp -- the key rule of the R plugin's duplicate count (Rgzfastq_uniq.c:164-203), which the kernels of rqc_dedup.hip and
// the host's ordering of clashing runs (hpn_rqcfile.hip) share.
//
// The plugin zeroes a 512-byte buffer per record and looks the C string in it up: mate 1 copies s1[0:50] when L1 > 75, else all
// of s1; mate 2 copies s2[0:50] to offset 50 when L2 > 75, else all of s2 to offset L1.  What the string then is:
//
//   single-end               s1[0:50] if L1 > 75, else s1
//   L2 > 75,  L1 < 50        s1                      (a NUL gap cuts mate 2 off)
//   L2 > 75,  L1 >= 50       s1[0:50] + s2[0:50]     (for 50 < L1 <= 75 mate 2 overwrites s1[50:])
//   L2 <= 75, L1 > 75        s1[0:50]                (mate 2 lands behind a NUL gap)
//   L2 <= 75, L1 <= 75       s1 + s2                 (no separator: AC/GT and ACG/T are one key)
//
// so a key is the first n0 bytes of mate 1's sequence and the first n1 of mate 2's: at most 150 bytes in two spans.
#pragma once
#include <hip/hip_runtime.h>

#include "sort_desc.hpp"

namespace hpn {

constexpr uint32_t kRqcMaxLen = 300;   // MaxLen: the matrices' columns
constexpr uint32_t kRqcHead = 50, kRqcWhole = 75;

__host__ __device__ inline void rqc_key_spans(uint32_t L1, uint32_t L2, int paired, uint32_t &n0, uint32_t &n1)
{
    n0 = L1 > kRqcWhole ? kRqcHead : L1, n1 = 0;
    if (!paired) return;
    if (L2 > kRqcWhole) {
        if (L1 >= kRqcHead) n0 = kRqcHead, n1 = kRqcHead;
    } else if (L1 <= kRqcWhole) {
        n1 = L2;
    }
}

}  // namespace hpn
