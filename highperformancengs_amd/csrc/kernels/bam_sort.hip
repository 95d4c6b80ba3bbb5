// bam_sort.hip -- samtools' coordinate sort on the device: the key of every record read in place, the keys' high words remapped
// to ranks so that the radix sort runs over the bits the keys use and no others, the sorted records' sizes for the scan that
// gives every output record its offset, and the gather that lays the records out in sorted order.  (docs/kernels/bam_sort.md)
//
//   k_sort_keys     per record, in place through rec_off[] (hpn_bam_raw_index_dev): block_size, refID, pos, the flag word ->
//                   the key (uint64_t)refID << 32 | (pos + 1) << 1 | strand of bam_sort.c's bam1_lt, the ordinal as payload, the
//                   size 4 + block_size, where the record lies in the session's store; the smallest and largest high word of
//                   either sign, the memory samtools would count for the record in a fresh slot, and the domain check
//                   -1 <= pos <= 2^30 - 2 through one atomicMin
//   k_sort_rank     the high words -> ranks that keep their unsigned order: refIDs from 0 up count from the smallest one, the
//                   negative ones (-1, and strays below it) follow from their smallest; the largest key for the bit range
//   k_sort_psize    psize[j] = size[order[j]]   (k_sort_psize_grown: + extra[order[j]], for records that grow on their way out)
//   k_sort_items    a slice of the sorted records as the items of the cut kernels (kernels/bam_split.hip): Q and key
//   k_sort_gather   16 lanes a record: record order[j] from the store to its place in the slice's payload
#include "bam_sort.hpp"
#include "common.hpp"

namespace hpn {

constexpr int kBsThreads = 256;
#ifdef HPN_TEST_HOOKS
constexpr unsigned kBsGatherBlocksPerCu = 0;    // (the test-hooks build: 16 workgroups in all, so that 4,097 records pass the grid's seam)
#else
constexpr unsigned kBsGatherBlocksPerCu = 8;
#endif

__device__ __forceinline__ u64 wave_min64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) v += __shfl_xor(v, d, kWave);
    return v;
}

__device__ __forceinline__ uint32_t bs_word(const uint8_t *q)      // (records are not aligned: bytes)
{
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
}

__global__ __launch_bounds__(kBsThreads) void k_sort_keys(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                          uint64_t base, uint64_t store_at, u64 *__restrict__ key, uint32_t *__restrict__ val,
                                                          uint32_t *__restrict__ size, u64 *__restrict__ soff, u64 *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
    const bool on = i < n;
    u64 bad = ~0ull, lo_min = ~0ull, lo_max = 0, hi_min = ~0ull, hi_max = 0, mem = 0;
    if (on) {
        const uint64_t first = rec_off[0], o = rec_off[i];
        const uint8_t *q = raw + o;
        const uint32_t bs = bs_word(q), tid = bs_word(q + 4), flag = bs_word(q + 16) >> 16;
        const int32_t pos = (int32_t)bs_word(q + 8);
        uint32_t reason = 0;
        if (pos < -1) reason = 1;                              // (pos + 1) << 1 floods the high word in bam1_lt and not in the merge's key
        else if (pos > (1 << 30) - 2) reason = 2;              // ... and overflows into the sign
        if (reason) bad = (base + i) << 3 | reason;
        const uint32_t low = (uint32_t)(pos + 1) << 1 | (flag >> 4 & 1u);
        key[base + i] = (u64)tid << 32 | low;
        val[base + i] = (uint32_t)(base + i);
        size[base + i] = bs + 4u;
        soff[base + i] = store_at + (o - first);
        if (tid < 0x80000000u) lo_min = tid, lo_max = (u64)tid + 1;
        else hi_min = tid, hi_max = (u64)tid - 0x7fffffffu;
        const uint32_t data_len = bs - 32u;
        uint32_t cap = data_len;                               // kroundup32
        if (cap) {
            --cap;
            cap |= cap >> 1, cap |= cap >> 2, cap |= cap >> 4, cap |= cap >> 8, cap |= cap >> 16;
            ++cap;
        }
        mem = 72ull + cap;
        if (i == 0) info[kBsFirst] = first;
        if (i == n - 1) info[kBsEnd] = o + 4 + (uint64_t)bs;
    }
    bad = wave_min64(bad), lo_min = wave_min64(lo_min), hi_min = wave_min64(hi_min);
    lo_max = wave_max64(lo_max), hi_max = wave_max64(hi_max), mem = wave_sum64(mem);
    if (lane_id() == 0) {
        if (bad != ~0ull) atomicMin(&info[kBsBad], bad);
        if (lo_max) atomicMin(&info[kBsLoMin], lo_min), atomicMax(&info[kBsLoMax], lo_max);
        if (hi_max) atomicMin(&info[kBsHiMin], hi_min), atomicMax(&info[kBsHiMax], hi_max);
        if (mem) atomicAdd(&info[kBsMem], mem);
    }
}

__global__ __launch_bounds__(kBsThreads) void k_sort_rank(u64 *__restrict__ key, uint64_t n, u64 *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
    const u64 lo_min = info[kBsLoMin], lo_max = info[kBsLoMax], hi_min = info[kBsHiMin];
    const u64 lo_count = lo_max ? lo_max - lo_min : 0;         // ranks the refIDs from 0 up take
    u64 k = 0;
    if (i < n) {
        const u64 old = key[i], h = old >> 32;
        const u64 rank = h < 0x80000000ull ? h - lo_min : lo_count + (h - hi_min);
        k = rank << 32 | (old & 0xffffffffull);
        key[i] = k;
    }
    k = wave_max64(k);
    if (lane_id() == 0 && k) atomicMax(&info[kBsMaxKey], k);
}

__global__ __launch_bounds__(kBsThreads) void k_sort_psize(const uint32_t *__restrict__ size, const uint32_t *__restrict__ order, uint64_t n,
                                                           uint32_t *__restrict__ psize)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
    if (j < n) psize[j] = size[order[j]];
}

__global__ __launch_bounds__(kBsThreads) void k_sort_psize_grown(const uint32_t *__restrict__ size, const uint32_t *__restrict__ extra,
                                                                 const uint32_t *__restrict__ order, uint64_t n, uint32_t *__restrict__ psize)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
    if (j < n) psize[j] = size[order[j]] + extra[order[j]];
}

// items of the slice [first, first + cnt) of the sorted records: item 0 the open block's `fill` bytes, item i + 1 record first + i
__global__ __launch_bounds__(kBsThreads) void k_sort_items(const u64 *__restrict__ out_off, uint64_t first, uint64_t cnt, uint32_t fill,
                                                           uint32_t open_key, u64 *__restrict__ Q, uint32_t *__restrict__ key)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
    if (i == 0) Q[0] = 0, key[0] = open_key, Q[1] = fill;
    if (i >= cnt) return;
    const u64 from = out_off[first];
    Q[i + 1] = (u64)fill + (out_off[first + i] - from);
    key[i + 1] = 0u;
    if (i == cnt - 1) Q[cnt + 1] = (u64)fill + (out_off[first + cnt] - from);
}

// One record by the 16 lanes of a team: `len` bytes from src to dst.  Where the two share their residue mod 16 both sides move
// in aligned 16-byte pieces, the head (up to dst's next 16-byte boundary) and the tail by bytes; otherwise the stores are
// aligned and the loads are not.  Every load lies inside [src, src + len), every store inside [dst, dst + len).
__device__ __forceinline__ void bs_copy_record(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t len, uint32_t sub)
{
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > len) head = len;
    const uint32_t vec = (len - head) / 16, tail0 = head + vec * 16;
    if (sub < head) dst[sub] = src[sub];
    u32 *dv = (u32 *)(dst + head);
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {
        const u32 *sv = (const u32 *)(src + head);
        for (uint32_t k = sub; k < vec; k += 16) dv[k] = load_stream16(sv + k);
    } else {
        const uint8_t *sp = src + head;
        for (uint32_t k = sub; k < vec; k += 16) {
            u32 v;
            __builtin_memcpy(&v, sp + 16 * (size_t)k, 16);
            dv[k] = v;
        }
    }
    if (tail0 + sub < len) dst[tail0 + sub] = src[tail0 + sub];      // (fewer than 16 bytes)
}

__global__ __launch_bounds__(kBsThreads) void k_sort_gather(const uint8_t *__restrict__ store, const u64 *__restrict__ soff,
                                                            const uint32_t *__restrict__ size, const uint32_t *__restrict__ order,
                                                            const u64 *__restrict__ out_off, uint64_t first, uint64_t cnt, uint8_t *__restrict__ pay)
{
    const uint64_t nwaves = (uint64_t)gridDim.x * (kBsThreads / kWave);
    const uint64_t wave = (uint64_t)blockIdx.x * (kBsThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    const u64 from = out_off[first];
    for (uint64_t k0 = wave * kWave; k0 < cnt; k0 += nwaves * kWave) {
        const uint64_t k = k0 + lane;
        u64 src = 0, dst = 0;
        uint32_t len = 0;
        if (k < cnt) {
            const uint32_t r = order[first + k];
            src = soff[r], len = size[r], dst = out_off[first + k] - from;
        }
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint64_t)it >= cnt) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t lj = __shfl(len, j, kWave);
            if (k0 + (uint64_t)j >= cnt) continue;
            bs_copy_record(store + sj, pay + dj, lj, (uint32_t)sub);
        }
    }
}

static inline unsigned bs_grid(uint64_t n) { return (unsigned)((n + kBsThreads - 1) / kBsThreads); }

hipError_t launch_bamsort_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, u64 *key, uint32_t *val,
                               uint32_t *size, u64 *soff, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_sort_keys, dim3(bs_grid(n)), dim3(kBsThreads), 0, st, raw, rec_off, n, base, store_at, key, val, size, soff, info);
    return hipGetLastError();
}

hipError_t launch_bamsort_rank(u64 *key, uint64_t n, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_sort_rank, dim3(bs_grid(n)), dim3(kBsThreads), 0, st, key, n, info);
    return hipGetLastError();
}

hipError_t launch_bamsort_psize(const uint32_t *size, const uint32_t *order, uint64_t n, uint32_t *psize, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_sort_psize, dim3(bs_grid(n)), dim3(kBsThreads), 0, st, size, order, n, psize);
    return hipGetLastError();
}

hipError_t launch_bamsort_psize_grown(const uint32_t *size, const uint32_t *extra, const uint32_t *order, uint64_t n, uint32_t *psize, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_sort_psize_grown, dim3(bs_grid(n)), dim3(kBsThreads), 0, st, size, extra, order, n, psize);
    return hipGetLastError();
}

hipError_t launch_bamsort_items(const u64 *out_off, uint64_t first, uint64_t cnt, uint32_t fill, uint32_t open_key, u64 *Q, uint32_t *key, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_items, dim3(cnt ? bs_grid(cnt) : 1u), dim3(kBsThreads), 0, st, out_off, first, cnt, fill, open_key, Q, key);
    return hipGetLastError();
}

hipError_t launch_bamsort_gather(const uint8_t *store, const u64 *soff, const uint32_t *size, const uint32_t *order, const u64 *out_off, uint64_t first,
                                 uint64_t cnt, uint8_t *pay, int n_cu, hipStream_t st)
{
    if (!cnt) return hipSuccess;
    const uint64_t want = (cnt + kBsThreads - 1) / kBsThreads;
    const uint64_t cap = kBsGatherBlocksPerCu ? (uint64_t)n_cu * kBsGatherBlocksPerCu : 16;
    hipLaunchKernelGGL(k_sort_gather, dim3((unsigned)(want < cap ? want : cap)), dim3(kBsThreads), 0, st, store, soff, size, order, out_off, first, cnt,
                       pay);
    return hipGetLastError();
}

}  // namespace hpn
