// uniq_desc.hpp -- the record descriptor of the device store behind hpn_fastq_uniq_* and hpn_fastq_uniqq_* (written by
// k_uniq_keys, kernels/fastq_uniq.hip) and the width of a count as "%u" prints it.
#pragma once
#include "common.hpp"

namespace hpn {

struct UniqDesc {
    u64 off;         // where the record's name line starts in the store
    u64 h0;          // sum of c[i] * B^(L-1-i) modulo 2^64 over the sequence
    uint32_t d0;     // the same with 33 modulo 2^32
    uint32_t sumq;   // sum of the first min(slen, qlen) quality bytes
    uint16_t nlen, slen, qlen, qrel;   // name, sequence, quality as the reference keeps them; quality's offset from `off`
};
static_assert(sizeof(UniqDesc) == 32, "UniqDesc is one 32-byte granule");

__device__ __forceinline__ uint32_t uniq_digits(uint32_t v)
{
    uint32_t d = 1;
    for (uint32_t p = 10; d < 10u && v >= p; p *= 10) ++d;
    return d;
}

}  // namespace hpn
