// sort_desc.hpp -- the record descriptor of the device store behind hpn_fastq_sort_*, hpn_twobit_pack_*, hpn_fastq_pair_*, hpn_mrle_* and hpn_rfastqc_*
// (written by k_sort_frame, kernels/fastq_sort.hip).  Plain C++: the kernels and the host (hpn_sort.hip, hpn_twobit.hip,
// hpn_pair.hip) read the same struct.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hpn {

struct SortDesc {
    unsigned long long off;            // where the record's name line starts in the store
    uint16_t nlen, slen, qlen, qrel;   // name, sequence, quality as the reference keeps them; quality's offset from `off`
};
constexpr size_t kSortDescBytes = 16;
static_assert(sizeof(SortDesc) == kSortDescBytes, "SortDesc is one 16-byte load");

}  // namespace hpn
