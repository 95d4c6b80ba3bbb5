// bam_merge.hip -- samtools' merge on the device: the heap's key of every record read in place, and the running maximum of the
// keys inside every input file, which turns the heap's output for ANY inputs into one stable sort.  (docs/kernels/bam_merge.md)
//
//   k_merge_keys      per record, in place through rec_off[] (hpn_bam_raw_index_dev): block_size, refID, pos, the flag word ->
//                     the key (uint64_t)refID << 32 | (uint32_t)(pos + 1) << 1 | strand of bam_merge_core2's heap -- the low word
//                     is cut to 32 bits, so every pos has its key --, the ordinal as payload, the number of the record's file, the
//                     size 4 + block_size, where the record lies in the session's store; the smallest and largest high word of
//                     either sign for k_sort_rank (kernels/bam_sort.hip); the one key the heap cannot hold, HEAP_EMPTY, through
//                     one atomicMin
//   the running maximum, restarted at every file: (file, key) pairs ordered by file first.  The file numbers never go down along
//   the store, so the plain running maximum of the pairs IS the segmented one of the keys -- a later file's first pair is above
//   everything in front of it -- and no head flags and no segmented operator exist.  Three launches, no workgroup waits for another:
//   k_merge_tilemax   the largest pair of every tile of 2,048 records
//   k_merge_tilescan  one workgroup: the tiles' maxima -> for every tile the largest pair in front of it
//   k_merge_apply     per tile: the scan inside it on top of what lies in front; key[i] <- the effective key, and the count of
//                     records whose effective key is not their own (0 exactly when every file was sorted)
#include "bam_merge.hpp"
#include "common.hpp"

namespace hpn {

namespace {

struct Pair {       // ordered by f, then k; {0, 0} is below or equal to every pair
    uint32_t f;
    u64 k;
};

__device__ __forceinline__ Pair pmax(Pair a, Pair b) { return (a.f > b.f || (a.f == b.f && a.k >= b.k)) ? a : b; }

__device__ __forceinline__ Pair wave_pmax(Pair v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        Pair o;
        o.f = __shfl_xor(v.f, d, kWave), o.k = __shfl_xor(v.k, d, kWave);
        v = pmax(v, o);
    }
    return v;
}

__device__ __forceinline__ u64 bm_wave_min64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 bm_wave_max64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t bm_word(const uint8_t *q)      // (records are not aligned: bytes)
{
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
}

constexpr int kBmWaves = kBmThreads / kWave;

}  // namespace

__global__ __launch_bounds__(kBmThreads) void k_merge_keys(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                           uint64_t base, uint64_t store_at, uint32_t file, u64 *__restrict__ key,
                                                           uint32_t *__restrict__ val, uint32_t *__restrict__ fid, uint32_t *__restrict__ size,
                                                           u64 *__restrict__ soff, u64 *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBmThreads + threadIdx.x;
    u64 bad = ~0ull, lo_min = ~0ull, lo_max = 0, hi_min = ~0ull, hi_max = 0;
    if (i < n) {
        const uint64_t first = rec_off[0], o = rec_off[i];
        const uint8_t *q = raw + o;
        const uint32_t bs = bm_word(q), tid = bm_word(q + 4), pos = bm_word(q + 8), flag = bm_word(q + 16) >> 16;
        const uint32_t low = (pos + 1u) << 1 | (flag >> 4 & 1u);
        const u64 k = (u64)tid << 32 | low;
        if (k == ~0ull) bad = (base + i) << 3 | 1u;            // HEAP_EMPTY: the reference ends its output at this record
        key[base + i] = k;
        val[base + i] = (uint32_t)(base + i);
        fid[base + i] = file;
        size[base + i] = bs + 4u;
        soff[base + i] = store_at + (o - first);
        if (tid < 0x80000000u) lo_min = tid, lo_max = (u64)tid + 1;
        else hi_min = tid, hi_max = (u64)tid - 0x7fffffffu;
        if (i == 0) info[kBsFirst] = first;
        if (i == n - 1) info[kBsEnd] = o + 4 + (uint64_t)bs;
    }
    bad = bm_wave_min64(bad), lo_min = bm_wave_min64(lo_min), hi_min = bm_wave_min64(hi_min);
    lo_max = bm_wave_max64(lo_max), hi_max = bm_wave_max64(hi_max);
    if (lane_id() == 0) {
        if (bad != ~0ull) atomicMin(&info[kBsBad], bad);
        if (lo_max) atomicMin(&info[kBsLoMin], lo_min), atomicMax(&info[kBsLoMax], lo_max);
        if (hi_max) atomicMin(&info[kBsHiMin], hi_min), atomicMax(&info[kBsHiMax], hi_max);
    }
}

__global__ __launch_bounds__(kBmThreads) void k_merge_tilemax(const u64 *__restrict__ key, const uint32_t *__restrict__ fid, uint64_t n,
                                                              uint32_t *__restrict__ tile_fid, u64 *__restrict__ tile_key)
{
    __shared__ uint32_t s_f[kBmWaves];
    __shared__ u64 s_k[kBmWaves];
    const uint64_t at = (uint64_t)blockIdx.x * kBmTile + (uint64_t)threadIdx.x * kBmPerThread;
    Pair m = {0u, 0ull};
#pragma unroll
    for (int j = 0; j < kBmPerThread; ++j)
        if (at + j < n) m = pmax(m, Pair{fid[at + j], key[at + j]});
    m = wave_pmax(m);
    if (lane_id() == 0) s_f[wave_id()] = m.f, s_k[wave_id()] = m.k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBmWaves; ++w) m = pmax(m, Pair{s_f[w], s_k[w]});
        tile_fid[blockIdx.x] = m.f, tile_key[blockIdx.x] = m.k;
    }
}

// One workgroup.  Thread t owns the tiles [t * per, (t + 1) * per); in place: a tile's maximum becomes the largest pair of all
// tiles in front of it ({0, 0} for tile 0).
__global__ __launch_bounds__(kBmThreads) void k_merge_tilescan(uint32_t *__restrict__ tile_fid, u64 *__restrict__ tile_key, uint64_t n_tiles)
{
    __shared__ uint32_t s_f[kBmThreads];
    __shared__ u64 s_k[kBmThreads];
    const uint64_t per = (n_tiles + kBmThreads - 1) / kBmThreads;
    const uint64_t from = (uint64_t)threadIdx.x * per, to = from + per < n_tiles ? from + per : n_tiles;
    Pair m = {0u, 0ull};
    for (uint64_t t = from; t < to; ++t) m = pmax(m, Pair{tile_fid[t], tile_key[t]});
    s_f[threadIdx.x] = m.f, s_k[threadIdx.x] = m.k;
    __syncthreads();
    if (threadIdx.x == 0) {
        Pair run = {0u, 0ull};
        for (int t = 0; t < kBmThreads; ++t) {
            const Pair own = {s_f[t], s_k[t]};
            s_f[t] = run.f, s_k[t] = run.k;
            run = pmax(run, own);
        }
    }
    __syncthreads();
    Pair run = {s_f[threadIdx.x], s_k[threadIdx.x]};
    for (uint64_t t = from; t < to; ++t) {
        const Pair own = {tile_fid[t], tile_key[t]};
        tile_fid[t] = run.f, tile_key[t] = run.k;
        run = pmax(run, own);
    }
}

__global__ __launch_bounds__(kBmThreads) void k_merge_apply(u64 *__restrict__ key, const uint32_t *__restrict__ fid, uint64_t n,
                                                            const uint32_t *__restrict__ tile_fid, const u64 *__restrict__ tile_key,
                                                            u64 *__restrict__ info)
{
    __shared__ uint32_t s_f[kBmWaves];
    __shared__ u64 s_k[kBmWaves];
    const uint64_t at = (uint64_t)blockIdx.x * kBmTile + (uint64_t)threadIdx.x * kBmPerThread;
    const int lane = lane_id(), wave = wave_id();
    Pair inc[kBmPerThread];      // the thread's eight records: the running maximum from its first one on
    u64 own[kBmPerThread];
    Pair run = {0u, 0ull};
#pragma unroll
    for (int j = 0; j < kBmPerThread; ++j) {
        own[j] = 0;
        if (at + j < n) own[j] = key[at + j], run = pmax(run, Pair{fid[at + j], own[j]});
        inc[j] = run;
    }
    // the threads' totals: inclusive over the wave, then what the lanes and the waves in front hold
    Pair w = run;
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        Pair o;
        o.f = __shfl_up(w.f, d, kWave), o.k = __shfl_up(w.k, d, kWave);
        if (lane >= d) w = pmax(w, o);
    }
    if (lane == kWave - 1) s_f[wave] = w.f, s_k[wave] = w.k;
    Pair before;
    before.f = __shfl_up(w.f, 1, kWave), before.k = __shfl_up(w.k, 1, kWave);
    if (lane == 0) before = Pair{0u, 0ull};
    __syncthreads();
    before = pmax(before, Pair{tile_fid[blockIdx.x], tile_key[blockIdx.x]});
    for (int v = 0; v < wave; ++v) before = pmax(before, Pair{s_f[v], s_k[v]});
    u64 lifted = 0;
#pragma unroll
    for (int j = 0; j < kBmPerThread; ++j) {
        if (at + j >= n) continue;
        const u64 eff = pmax(before, inc[j]).k;                // (the largest pair up to a record is of the record's own file)
        if (eff != own[j]) key[at + j] = eff, ++lifted;
    }
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) lifted += __shfl_xor(lifted, d, kWave);
    if (lane == 0 && lifted) atomicAdd(&info[kBmLifted], lifted);
}

hipError_t launch_bammerge_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, uint32_t file, u64 *key,
                                uint32_t *val, uint32_t *fid, uint32_t *size, u64 *soff, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_merge_keys, dim3((unsigned)((n + kBmThreads - 1) / kBmThreads)), dim3(kBmThreads), 0, st, raw, rec_off, n, base, store_at, file, key,
                       val, fid, size, soff, info);
    return hipGetLastError();
}

hipError_t launch_bammerge_runmax(u64 *key, const uint32_t *fid, uint64_t n, uint32_t *tile_fid, u64 *tile_key, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    const uint64_t tiles = bammerge_tiles(n);      // (below 2^31 records: at most 2^20 tiles)
    hipLaunchKernelGGL(k_merge_tilemax, dim3((unsigned)tiles), dim3(kBmThreads), 0, st, key, fid, n, tile_fid, tile_key);
    hipLaunchKernelGGL(k_merge_tilescan, dim3(1), dim3(kBmThreads), 0, st, tile_fid, tile_key, tiles);
    hipLaunchKernelGGL(k_merge_apply, dim3((unsigned)tiles), dim3(kBmThreads), 0, st, key, fid, n, tile_fid, tile_key, info);
    return hipGetLastError();
}

}  // namespace hpn
