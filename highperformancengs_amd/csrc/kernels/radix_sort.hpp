// radix_sort.hpp -- device-wide exclusive scan and a stable LSD radix sort of 64-bit keys with a 32-bit
// payload for gfx950 (wave64).  No library underneath: the digit offsets come from scan.hpp's look-back.
//
//   k_excl_scan      out[i] = sum of in[0 .. i), out[n] = the total.  One workgroup = one tile of kScanTile
//                    items taken in ticket order, one look-back hand-off per tile.
//   k_radix_hist     one WAVE = one tile of kSortTile keys: 256-bin histogram of the pass's digit in LDS
//                    (ds_add), written bin-major -- hist[digit * tiles + tile] -- so that ONE linear scan of
//                    the matrix gives every (digit, tile) its first output position.
//   k_radix_scatter  the same tiles: a wave walks its tile 64 keys at a time in order; lanes with the same
//                    digit find each other with eight ballots, a key's place is base[digit] (LDS) + the
//                    number of equal digits in lower lanes, the highest such lane then moves base[digit].
//                    Earlier keys always land in front of later equal ones: the sort is stable.
//
// A pass reads keys + payload twice and writes them once; passes over digits that cannot differ are left out
// by the caller through [begin_bit, end_bit).  Bound: HBM (12 B read twice, written once, per key and pass);
// the scatter's stores are 12-byte pieces in up to 256 streams per tile, which is what keeps it under that.
#pragma once
#include "scan.hpp"

namespace hpn {

constexpr int kSortThreads = 256;                              // four tiles per workgroup
constexpr uint32_t kSortRounds = 32;
constexpr uint32_t kSortTile = kWave * kSortRounds;             // 2048 keys per wave
constexpr int kScanThreads = 256;
constexpr uint32_t kScanItems = 8;
constexpr uint32_t kScanTile = kScanThreads * kScanItems;       // 2048 items per workgroup

// ticket: one word, zeroed by the launcher; err: set (never cleared here) when a look-back hand-off timed out
template <typename TIn, typename TOut>
__global__ __launch_bounds__(kScanThreads) void k_excl_scan(const TIn *__restrict__ in, TOut *__restrict__ out, uint64_t n,
                                                           u64 *__restrict__ status, uint32_t *__restrict__ ticket,
                                                           uint32_t *__restrict__ err)
{
    __shared__ u64 s_wave[kScanThreads / kWave];
    __shared__ u64 s_excl;
    __shared__ uint32_t s_tile;
    const int tid = threadIdx.x;
    if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint64_t tile = s_tile;
    const uint64_t i0 = tile * kScanTile + (uint64_t)tid * kScanItems;
    u64 v[kScanItems], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        v[k] = i0 + k < n ? (u64)in[i0 + k] : 0;
        mine += v[k];
    }
    u64 wtotal;
    const u64 wexcl = wave_excl_scan(mine, wtotal);
    if (lane_id() == kWave - 1) s_wave[wave_id()] = wtotal;
    __syncthreads();
    u64 before = 0, aggregate = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / kWave; ++w) {
        if (w < wave_id()) before += s_wave[w];
        aggregate += s_wave[w];
    }
    if (wave_id() == 0) {
        const u64 ex = scan_lookback(status, tile, aggregate, err);
        if (lane_id() == 0) s_excl = ex;
    }
    __syncthreads();
    u64 run = s_excl + before + wexcl;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (i0 + k < n) out[i0 + k] = (TOut)run;
        run += v[k];
        if (i0 + k + 1 == n) out[n] = (TOut)run;
    }
    if (n == 0 && tile == 0 && tid == 0) out[0] = 0;
}

inline uint64_t scan_tiles(uint64_t n) { return n / kScanTile + 1; }

// d_status: scan_tiles(n) words and d_ticket are zeroed here; d_err is the caller's.  out has n + 1 entries.
template <typename TIn, typename TOut>
hipError_t launch_excl_scan(const TIn *d_in, TOut *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t s)
{
    const uint64_t t = scan_tiles(n);
    hipError_t e = hipMemsetAsync(d_status, 0, t * sizeof(u64), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_ticket, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_excl_scan<TIn, TOut>), dim3((unsigned)t), dim3(kScanThreads), 0, s, d_in, d_out, n, d_status, d_ticket, d_err);
    return hipGetLastError();
}

__global__ __launch_bounds__(kSortThreads) void k_radix_hist(const uint64_t *__restrict__ keys, uint32_t n, int shift,
                                                             uint32_t mask, uint32_t tiles, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_h[kSortThreads / kWave][256];
    const int w = wave_id(), lane = lane_id();
    const uint32_t tile = blockIdx.x * (kSortThreads / kWave) + (uint32_t)w;
    for (int b = lane; b < 256; b += kWave) s_h[w][b] = 0;
    __syncthreads();
    if (tile < tiles) {
        const uint32_t i0 = tile * kSortTile;
        for (uint32_t r = 0; r < kSortRounds; ++r) {
            const uint32_t i = i0 + r * kWave + (uint32_t)lane;
            if (i < n) atomicAdd(&s_h[w][(uint32_t)(keys[i] >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    if (tile < tiles)
        for (int b = lane; b < 256; b += kWave) hist[(size_t)b * tiles + tile] = s_h[w][b];
}

__global__ __launch_bounds__(kSortThreads) void k_radix_scatter(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                uint32_t n, int shift, uint32_t mask, uint32_t tiles,
                                                                const uint32_t *__restrict__ offs, uint64_t *__restrict__ keys_out,
                                                                uint32_t *__restrict__ vals_out)
{
    __shared__ uint32_t s_base[kSortThreads / kWave][256];
    const int w = wave_id(), lane = lane_id();
    const uint32_t tile = blockIdx.x * (kSortThreads / kWave) + (uint32_t)w;
    const bool live = tile < tiles;
    if (live)
        for (int b = lane; b < 256; b += kWave) s_base[w][b] = offs[(size_t)b * tiles + tile];
    __syncthreads();
    const uint32_t i0 = tile * kSortTile;
    const u64 below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < kSortRounds; ++r) {   // (every wave of the workgroup makes all rounds: the barriers are uniform)
        const uint32_t i = i0 + r * kWave + (uint32_t)lane;
        const bool have = live && i < n;
        uint64_t k = 0;
        uint32_t v = 0, d = 0;
        if (have) k = keys[i], v = vals[i], d = (uint32_t)(k >> shift) & mask;
        u64 same = __ballot(have);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 m = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? m : ~m;
        }
        uint32_t base = 0;
        if (have) base = s_base[w][d];
        __syncthreads();
        if (have) {
            const uint32_t rank = (uint32_t)__builtin_popcountll(same & below);
            const uint32_t p = base + rank;
            if (p < n) keys_out[p] = k, vals_out[p] = v;   // (p < n always: the guard keeps a damaged table from writing outside)
            if ((same >> lane) == 1ull) s_base[w][d] = base + rank + 1u;   // the highest lane with this digit
        }
        __syncthreads();
    }
}

inline uint32_t sort_tiles(uint32_t n) { return (n + kSortTile - 1) / kSortTile; }
inline size_t sort_hist_words(uint32_t n) { return (size_t)256 * sort_tiles(n) + 1; }

// Work space of one sort of up to n keys: the second copy of keys and payload, the histogram matrix (twice:
// counts and their scan), the scan's look-back words and state.
struct SortSpace {
    uint64_t *keys_tmp;
    uint32_t *vals_tmp;
    uint32_t *hist, *offs;   // sort_hist_words(n) each
    u64 *status;             // scan_tiles(sort_hist_words(n))
    uint32_t *ticket, *err;  // one word each (err: see k_excl_scan)
};

// Sorts (keys, vals) by the key bits [begin_bit, end_bit) in place (stable) and by no others: the last pass's digit is as wide
// as what is left of the range.
inline hipError_t radix_sort_pairs(uint64_t *d_keys, uint32_t *d_vals, uint32_t n, int begin_bit, int end_bit, const SortSpace &ws,
                                   hipStream_t s)
{
    if (n < 2 || end_bit <= begin_bit) return hipSuccess;
    const uint32_t tiles = sort_tiles(n);
    const unsigned grid = (tiles + kSortThreads / kWave - 1) / (kSortThreads / kWave);
    const size_t hw = (size_t)256 * tiles;
    uint64_t *ka = d_keys, *kb = ws.keys_tmp;
    uint32_t *va = d_vals, *vb = ws.vals_tmp;
    int pass = 0;
    for (int shift = begin_bit; shift < end_bit; shift += 8, ++pass) {
        const uint32_t mask = (1u << (end_bit - shift < 8 ? end_bit - shift : 8)) - 1u;
        hipLaunchKernelGGL(k_radix_hist, dim3(grid), dim3(kSortThreads), 0, s, ka, n, shift, mask, tiles, ws.hist);
        hipError_t e = launch_excl_scan<uint32_t, uint32_t>(ws.hist, ws.offs, hw, ws.status, ws.ticket, ws.err, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_radix_scatter, dim3(grid), dim3(kSortThreads), 0, s, ka, va, n, shift, mask, tiles, ws.offs, kb, vb);
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    if (ka != d_keys) {
        hipError_t e = hipMemcpyAsync(d_keys, ka, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_vals, va, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace hpn
