// fastq_uniqq.hip -- gfx950 kernels of hpn_fastq_uniqq_* (gzfastq_uniqQ.c on the device).
//
// The reference keys a chained hash table by the sequence like gzfastq_uniq.c, but keeps EVERY record's name and quality in a
// list per key, new records at the head (list_add_data, list.c), and prints per key
//     name of the head \t count \n sequence \n + \n        (gzfastq_uniqQ.c:86)
// and then every member's quality line, head to tail (:67-76) -- the last record read first.  The keys come in sdscmp order
// (-S) or by count descending through a stable qsort over the table walk (-C, :242-259).
//
// The grouping stage is gzfastq_uniq's (hpn_uniq_group.hpp): order[] holds the record ordinals sorted stably by grouping hash,
// so the members of a group lie side by side at the sorted positions [s, e), ascending by ordinal; the head of the reference's
// list is the member at e - 1.  One group may hold most of the file, so nothing here walks a group:
//
//   k_uniqq_len      per sorted position p: len[p] = quality length + 1; where a group opens: start[group] = p, and the greatest
//                    count of all (atomicMax).  A device-wide scan with 64-bit sums gives P[] (P[N]: all quality lines;
//                    uniq_scan64 and uniq_scan64w, kernels/fastq_uniq.hip).
//   k_uniqq_sizes    per output position q (group list[q]): header bytes + P[e] - P[s].  A 64-bit scan gives the group offsets.
//   k_uniqq_base     per output position: base[group] = offset + header bytes + P[e], so that the member at p writes its
//                    quality line to base[group] - P[p + 1]: the member at e - 1 first, the one at s last.
//   k_uniqq_count_key  the -C sort key: (0xffffffff - count) << 32 | position in the table walk.
//   k_uniqq_write    16 lanes per RECORD (copy_span): its quality line; the member at e - 1 also writes the header in front
//                    of its own line.  Work per team is bounded by one record however large a group is.
//
// Bound: HBM.  len reads 32 B per record through the sorted order and writes 4 B; the scan reads 4 B and writes 8 B per
// record; sizes and base read one descriptor per group; write reads per record its descriptor, 24 B of indices and its
// quality line (per group the name and the sequence as well) and writes the output once.
#include "text_common.hpp"
#include "uniq_desc.hpp"

namespace hpn {

// "%s\t%u\n%s\n+\n" in front of the quality lines
__device__ __forceinline__ uint32_t uniqq_header(const UniqDesc &d, uint32_t count)
{
    return (uint32_t)d.nlen + 1u + uniq_digits(count) + 1u + (uint32_t)d.slen + 3u;
}

__global__ __launch_bounds__(256) void k_uniqq_len(const UniqDesc *__restrict__ desc, const uint32_t *__restrict__ order,
                                                   const uint32_t *__restrict__ flag, const uint32_t *__restrict__ gid,
                                                   const uint32_t *__restrict__ count, uint32_t n, uint32_t *__restrict__ len,
                                                   uint32_t *__restrict__ start, uint32_t *__restrict__ max_count)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = 0;
    if (p < n) {
        len[p] = (uint32_t)desc[order[p]].qlen + 1u;
        if (flag[p]) {
            const uint32_t g = gid[p];
            start[g] = p;
            c = count[g];
        }
    }
    const uint32_t m = wave_max(c);
    if (lane_id() == 0 && m) atomicMax(max_count, m);
}

__global__ __launch_bounds__(256) void k_uniqq_sizes(const UniqDesc *__restrict__ desc, const uint32_t *__restrict__ order,
                                                     const uint32_t *__restrict__ list, const uint32_t *__restrict__ start,
                                                     const uint32_t *__restrict__ count, const uint64_t *__restrict__ P,
                                                     uint32_t n_groups, uint64_t *__restrict__ total)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_groups) return;
    const uint32_t g = list[q], s = start[g], c = count[g], e = s + c;
    total[q] = (u64)uniqq_header(desc[order[e - 1u]], c) + (P[e] - P[s]);
}

__global__ __launch_bounds__(256) void k_uniqq_base(const UniqDesc *__restrict__ desc, const uint32_t *__restrict__ order,
                                                    const uint32_t *__restrict__ list, const uint32_t *__restrict__ start,
                                                    const uint32_t *__restrict__ count, const uint64_t *__restrict__ P,
                                                    const uint64_t *__restrict__ goff, uint32_t n_groups, uint64_t *__restrict__ base)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_groups) return;
    const uint32_t g = list[q], c = count[g], e = start[g] + c;
    base[g] = goff[q] + (u64)uniqq_header(desc[order[e - 1u]], c) + P[e];
}

// The walk's array is the sort's input, so the low word is ascending already and a stable sort of the high word's digits
// alone leaves equal counts in the order of the walk -- what glibc's merge sort does to dump_dict's array.
__global__ __launch_bounds__(256) void k_uniqq_count_key(const uint32_t *__restrict__ list_table, const uint32_t *__restrict__ count,
                                                         uint32_t n_groups, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_groups) return;
    const uint32_t g = list_table[q];
    key[q] = ((u64)(0xffffffffu - count[g]) << 32) | q;
    val[q] = g;
}

__global__ __launch_bounds__(kTxtThreads) void k_uniqq_write(const uint8_t *__restrict__ text, const UniqDesc *__restrict__ desc,
                                                             const uint32_t *__restrict__ order, const uint32_t *__restrict__ flag,
                                                             const uint32_t *__restrict__ gid, const uint32_t *__restrict__ count,
                                                             const uint64_t *__restrict__ P, const uint64_t *__restrict__ base,
                                                             uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t p0 = wave * kWave; p0 < n; p0 += nwaves * kWave) {
        const uint32_t p = p0 + lane;
        u64 src = 0, dst = 0;
        uint32_t nlen = 0, slen = 0, qlen = 0, qrel = 0, hdr = 0;   // nlen, slen, hdr: of the group's last member only
        if (p < n) {
            const uint32_t f = flag[p], g = gid[p] + f - 1u;
            const UniqDesc d = desc[order[p]];
            src = d.off, qlen = d.qlen, qrel = d.qrel;
            dst = base[g] - P[p + 1u];   // where the quality line goes
            out[dst + qlen] = '\n';
            if (p + 1u == n || flag[p + 1u]) {   // the head of the reference's list: the header, by the record's own lane
                uint32_t c = count[g];
                const uint32_t nd = uniq_digits(c);
                nlen = d.nlen, slen = d.slen;
                hdr = nlen + 1u + nd + 1u + slen + 3u;
                uint8_t *o = out + (dst - hdr) + nlen;
                o[0] = '\t';
                for (uint32_t i = nd; i > 0; --i) o[i] = (uint8_t)('0' + c % 10u), c /= 10u;
                o[nd + 1u] = '\n';
                o += nd + 2u + slen;
                o[0] = '\n', o[1] = '+', o[2] = '\n';
            }
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (p0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), cj = __shfl(slen, j, kWave), mj = __shfl(qlen, j, kWave);
            const uint32_t rj = __shfl(qrel, j, kWave), hj = __shfl(hdr, j, kWave);
            if (p0 + (uint32_t)j >= n) continue;
            copy_span(text + sj + rj, out + dj, mj, sub);
            if (hj) {
                uint8_t *o = out + (dj - hj);
                copy_span(text + sj, o, nj, sub);
                copy_span(text + sj + nj + 1u, o + (hj - 3u - cj), cj, sub);
            }
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned blocks256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }

hipError_t launch_uniqq_len(const void *d_desc, const uint32_t *d_order, const uint32_t *d_flag, const uint32_t *d_gid,
                            const uint32_t *d_count, uint32_t n, uint32_t *d_len, uint32_t *d_start, uint32_t *d_max_count, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniqq_len, dim3(blocks256(n)), dim3(256), 0, st, (const UniqDesc *)d_desc, d_order, d_flag, d_gid, d_count, n, d_len,
                       d_start, d_max_count);
    return hipGetLastError();
}

hipError_t launch_uniqq_sizes(const void *d_desc, const uint32_t *d_order, const uint32_t *d_list, const uint32_t *d_start,
                              const uint32_t *d_count, const uint64_t *d_P, uint32_t n_groups, uint64_t *d_total, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniqq_sizes, dim3(blocks256(n_groups)), dim3(256), 0, st, (const UniqDesc *)d_desc, d_order, d_list, d_start, d_count,
                       d_P, n_groups, d_total);
    return hipGetLastError();
}

hipError_t launch_uniqq_base(const void *d_desc, const uint32_t *d_order, const uint32_t *d_list, const uint32_t *d_start,
                             const uint32_t *d_count, const uint64_t *d_P, const uint64_t *d_goff, uint32_t n_groups, uint64_t *d_base,
                             hipStream_t st)
{
    hipLaunchKernelGGL(k_uniqq_base, dim3(blocks256(n_groups)), dim3(256), 0, st, (const UniqDesc *)d_desc, d_order, d_list, d_start, d_count,
                       d_P, d_goff, n_groups, d_base);
    return hipGetLastError();
}

hipError_t launch_uniqq_count_key(const uint32_t *d_list_table, const uint32_t *d_count, uint32_t n_groups, uint64_t *d_key, uint32_t *d_val,
                                  hipStream_t st)
{
    hipLaunchKernelGGL(k_uniqq_count_key, dim3(blocks256(n_groups)), dim3(256), 0, st, d_list_table, d_count, n_groups, d_key, d_val);
    return hipGetLastError();
}

hipError_t launch_uniqq_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_order, const uint32_t *d_flag,
                              const uint32_t *d_gid, const uint32_t *d_count, const uint64_t *d_P, const uint64_t *d_base, uint32_t n,
                              uint8_t *d_out, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t want = ((uint64_t)n + kTxtThreads - 1) / kTxtThreads, cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_uniqq_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, d_text, (const UniqDesc *)d_desc,
                       d_order, d_flag, d_gid, d_count, d_P, d_base, n, d_out);
    return hipGetLastError();
}

}  // namespace hpn
