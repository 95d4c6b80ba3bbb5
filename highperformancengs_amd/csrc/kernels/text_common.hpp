// text_common.hpp -- what the kernels of the raw-text front end share (fastq_text.hip, fastq_sample.hip).
#pragma once
#include "scan.hpp"

namespace hpn {

constexpr int kTxtThreads = 256;

// device state block (uint32 words), zeroed before every chunk
enum { kTsLines = 0, kTsRecs, kTsFlags, kTsUnterminated, kTsConsumed, kTsTotalLo, kTsTotalHi, kTsErr, kTsTicket1, kTsTicket2, kTsOwnLines, kTsKept, kTsWords = 16 };

// 16 lanes copy one span: 16-byte unaligned pieces, the last one overlapping its
// predecessor; spans shorter than 16 bytewise.
__device__ __forceinline__ void copy_span(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t cnt, int sub)
{
    if (cnt >= 16u) {
        for (uint32_t i = 16u * (uint32_t)sub; i < cnt; i += 256u) {
            const uint32_t o = min(i, cnt - 16u);
            u32 v;
            __builtin_memcpy(&v, src + o, 16);
            __builtin_memcpy(dst + o, &v, 16);
        }
    } else if ((uint32_t)sub < cnt) {
        dst[sub] = src[sub];
    }
}

}  // namespace hpn
