// bam_bai.hip -- samtools' `index` on the device: bam_index_core's pass over the records (bam_index.c), read where they lie in
// the inflated stream through rec_off[] of hpn_bam_raw_index_dev.  (docs/kernels/bam_bai.md)
//
//   k_bai_records   per record: refID, pos, stored bin, flag, the CIGAR's end on the reference; the record's START offset -- the
//                   virtual offset behind the record before it: a binary search of that stream position in the call's block
//                   table --; order and domain checks (the lowest offending ordinal through one atomicMin); whether a run of
//                   equal (refID, bin) starts here; per wave and target the mapped / unmapped counts and the last mapped
//                   record's window count (one atomic each); the linear index's minima (64-bit atomicMin, a window the record
//                   before already covers is skipped: offsets ascend in file order)
//   k_bai_count / k_bai_tiles / k_bai_emit   the run heads compacted in file order into {start offset, bin, refID}
//   k_bai_fill      at the end: empty windows take the offset to their left, a workgroup per target
// A chunk ends where the next run starts, so the lists, their merge and their order are made of the heads alone (hpn_bai.hip).
#include "common.hpp"
#include "scan.hpp"

namespace hpn {

constexpr int kBaiThreads = 256;
#ifdef HPN_TEST_HOOKS
constexpr uint32_t kBaiTile = 64;               // (the test-hooks build: small batches cross tiles)
#else
constexpr uint32_t kBaiTile = 4096;             // records per workgroup in the scan of the head counts
#endif
constexpr u64 kBaiEmpty = ~0ull;                // a window no record has reached

struct BaiBlock {        // hpn_bgzf_block
    uint64_t in_off;
    uint32_t in_len, out_len;
    uint64_t out_off;
};

struct BaiState {        // carried from call to call on the device (two of them, used in turn)
    int32_t tid, pos;
    uint32_t bin, have;
    u64 last_end;        // the virtual offset behind the last record: where the next one starts
};

struct BaiHead {         // 16 bytes
    u64 start;
    uint32_t bin;
    int32_t tid;
};

// n 32-bit words from an address of any alignment: n + 1 aligned loads (the word behind the last one is read as well: it lies
// inside the record, or inside the 16 bytes the stream is readable past its end)
template <int N>
__device__ __forceinline__ void bai_words(const uint8_t *p, uint32_t *out)
{
    const uint32_t *a = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3) * 8;
    uint32_t lo = a[0];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t hi = a[k + 1];
        out[k] = __funnelshift_r(lo, hi, sh);
        lo = hi;
    }
}

// What bam_tell says with the stream consumed up to position p (p lies behind a record: p > blk[0].out_off): the block holding
// byte p - 1 is the last one that starts before p (a block of no bytes shares its start with the block behind it and is never
// that one); consumed to its end, the reader already stands at the next block's address.
__device__ __forceinline__ u64 bai_voffset(const BaiBlock *__restrict__ blk, const u64 *__restrict__ addr, uint32_t nb, u64 p)
{
    uint32_t lo = 0, hi = nb;                    // first block with out_off >= p
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (blk[mid].out_off >= p) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t k = lo ? lo - 1 : 0;
    const u64 within = p - blk[k].out_off;
    return within >= blk[k].out_len ? addr[k + 1] << 16 : addr[k] << 16 | within;
}

// info (u64 words): [0] lowest (ordinal << 4 | reason), ~0 none   [1] records without a refID   [2] run heads (k_bai_tiles)
__global__ __launch_bounds__(kBaiThreads) void k_bai_records(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                             int32_t n_ref, uint64_t base, const BaiBlock *__restrict__ blk,
                                                             const u64 *__restrict__ addr, uint32_t nb, const int32_t *__restrict__ target_len,
                                                             const u64 *__restrict__ win_base, const BaiState *__restrict__ prev,
                                                             BaiState *__restrict__ next, uint8_t *__restrict__ head, u64 *__restrict__ counts,
                                                             u64 *__restrict__ last_mapped, u64 *__restrict__ lin, u64 *__restrict__ info)
{
    __shared__ int32_t s_tid[kBaiThreads], s_pos[kBaiThreads];
    __shared__ uint32_t s_bf[kBaiThreads];           // bin << 16 | flag
    const uint64_t i = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
    const bool live = i < n;
    int32_t tid = -1, pos = 0;
    uint32_t bin = 0, flag = 4, l_name = 0, n_cigar = 0, bsize = 0;
    uint64_t o = 0;
    if (live) {
        o = rec_off[i];
        uint32_t w[5];                               // block_size, refID, pos, bin_mq_nl, flag_nc
        bai_words<5>(raw + o, w);
        bsize = w[0], tid = (int32_t)w[1], pos = (int32_t)w[2];
        bin = w[3] >> 16, l_name = w[3] & 0xffu, flag = w[4] >> 16, n_cigar = w[4] & 0xffffu;
    }
    s_tid[threadIdx.x] = tid, s_pos[threadIdx.x] = pos, s_bf[threadIdx.x] = bin << 16 | flag;
    __syncthreads();
    int32_t ptid = -1, ppos = 0;
    uint32_t pbin = 0, pflag = 4;
    bool have = false;
    if (live) {
        if (i == 0) {
            ptid = prev->tid, ppos = prev->pos, pbin = prev->bin, have = prev->have != 0;
        } else if (threadIdx.x) {
            ptid = s_tid[threadIdx.x - 1], ppos = s_pos[threadIdx.x - 1], pbin = s_bf[threadIdx.x - 1] >> 16, pflag = s_bf[threadIdx.x - 1] & 0xffffu;
            have = true;
        } else {
            uint32_t w[4];                           // refID, pos, bin_mq_nl, flag_nc of the record before
            bai_words<4>(raw + rec_off[i - 1] + 4, w);
            ptid = (int32_t)w[0], ppos = (int32_t)w[1], pbin = w[2] >> 16, pflag = w[3] >> 16;
            have = true;
        }
    }
    const bool placed = live && tid >= 0 && tid < n_ref;
    const bool mapped = placed && !(flag & 4u);
    uint32_t reason = 0;
    if (live) {
        if (tid < -1 || tid >= n_ref) reason = 1;                                    // refID outside the header's targets
        else if (mapped && pos < 0) reason = 2;                                      // a mapped record in front of the reference
        else if (have && (uint32_t)tid < (uint32_t)ptid) reason = 3;                 // refID goes backwards (-1 sorts last)
        else if (have && tid == ptid && tid >= 0 && pos < ppos) reason = 4;          // pos goes backwards inside a target
        else if (tid >= 0 && bin == 37450u) reason = 7;                              // the stored bin is the metadata bin's number
        else if (32u + l_name + 4u * n_cigar > bsize) reason = 8;                    // name and CIGAR do not fit the record
    }
    // the CIGAR's end on the reference and the windows the record reaches
    int32_t beg_w = 0, end_w = -1;
    uint32_t n_win = 0;
    if (mapped && !reason) {
        const uint8_t *cg = raw + o + 36 + l_name;
        const uint32_t *a = (const uint32_t *)((uintptr_t)cg & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)((uintptr_t)cg & 3) * 8;
        uint32_t end = (uint32_t)pos, lo = n_cigar ? a[0] : 0u;
        bool back = false;
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t hi = a[k + 1], c = __funnelshift_r(lo, hi, sh), op = c & 15u;
            lo = hi;
            if (op == 9u) back = true;
            if (0x3C1A7u >> (op << 1) & 2u) end += c >> 4;                           // M D N = X consume the reference
        }
        const int32_t len = target_len[tid];
        n_win = len > 0 ? (uint32_t)((len - 1) >> 14) + 1u : 0u;
        beg_w = pos >> 14, end_w = (int32_t)((end - 1u) >> 14);
        if (back) reason = 6;                                                        // a `B` operation moves the end backwards
        else if (end < (uint32_t)pos) reason = 5;                                    // (the end wrapped past 2^32)
        else if ((uint32_t)end_w >= n_win) reason = 5;                               // a window the target does not have
    }
    if (reason) atomicMin(&info[0], (u64)((base + i) << 4 | reason));
    const bool ok = live && !reason;
    // where the record starts: behind the record before it
    u64 start = 0;
    const bool is_head = ok && (!have || tid != ptid || (tid >= 0 && bin != pbin));
    if (ok && (mapped || is_head)) start = i == 0 ? prev->last_end : bai_voffset(blk, addr, nb, o);
    if (live) head[i] = is_head ? 1 : 0;
    if (mapped && ok) {
        // A window the record before it has reached holds a smaller offset already: the record before is of the same target,
        // mapped, starts in the same window and not on its first base (so even without a CIGAR it reaches that window).
        int32_t w = beg_w;
        if (i != 0 && have && ptid == tid && !(pflag & 4u) && ppos >= 0 && (ppos >> 14) == beg_w && (ppos & 16383)) ++w;
        u64 *row = lin + win_base[tid];
        for (; w <= end_w; ++w) atomicMin(&row[w], start);
    }
    // per wave: the counts of every target present, the last mapped record of each, the records without a refID
    const int lane = lane_id();
    const bool counted = ok && tid >= 0;
    u64 todo = __ballot(counted);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int32_t t = __shfl(tid, lead, kWave);
        const u64 same = __ballot(counted && tid == t), m = __ballot(counted && tid == t && mapped);
        if (lane == lead) {
            if (m) atomicAdd(&counts[2 * (size_t)t], (u64)__builtin_popcountll(m));
            if (same != m) atomicAdd(&counts[2 * (size_t)t + 1], (u64)__builtin_popcountll(same & ~m));
        }
        if (m && lane == 63 - __builtin_clzll(m)) atomicMax(&last_mapped[t], (u64)((base + i + 1) << 20 | (uint32_t)(end_w + 1)));
        todo &= ~same;
    }
    const u64 loose = __ballot(ok && tid < 0);
    if (loose && lane == __builtin_ctzll(loose)) atomicAdd(&info[1], (u64)__builtin_popcountll(loose));
    if (live && i == n - 1) {
        next->tid = tid, next->pos = pos, next->bin = bin, next->have = 1u;
        next->last_end = bai_voffset(blk, addr, nb, o + 4 + (uint64_t)bsize);
    }
}

// tile_sum[t] = run heads of tile t
__global__ __launch_bounds__(kBaiThreads) void k_bai_count(const uint8_t *__restrict__ head, uint64_t n, u64 *__restrict__ tile_sum)
{
    __shared__ uint32_t part[kBaiThreads / kWave];
    const uint64_t t0 = (uint64_t)blockIdx.x * kBaiTile;
    uint32_t mine = 0;
    for (uint32_t k = threadIdx.x; k < kBaiTile; k += kBaiThreads)
        if (t0 + k < n) mine += head[t0 + k];
    mine = wave_sum(mine);
    if (lane_id() == 0) part[wave_id()] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int w = 0; w < kBaiThreads / kWave; ++w) s += part[w];
        tile_sum[blockIdx.x] = s;
    }
}

// exclusive scan of the tile sums in place (one workgroup), the total into info[2]
__global__ __launch_bounds__(1024) void k_bai_tiles(u64 *__restrict__ tile_sum, uint32_t n_tiles, u64 *__restrict__ info)
{
    __shared__ u64 part[1024];
    const uint32_t per = (n_tiles + 1023) / 1024, a0 = threadIdx.x * per, a = a0 < n_tiles ? a0 : n_tiles, b = a + per < n_tiles ? a + per : n_tiles;
    u64 s = 0;
    for (uint32_t t = a; t < b; ++t) s += tile_sum[t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = 0;
        for (int k = 0; k < 1024; ++k) {
            const u64 v = part[k];
            part[k] = run, run += v;
        }
        info[2] = run;
    }
    __syncthreads();
    u64 run = part[threadIdx.x];
    for (uint32_t t = a; t < b; ++t) {
        const u64 v = tile_sum[t];
        tile_sum[t] = run, run += v;
    }
}

// the heads in file order: one wave per tile, 64 records at a time
__global__ __launch_bounds__(kWave) void k_bai_emit(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, const uint8_t *__restrict__ head,
                                                    uint64_t n, const BaiBlock *__restrict__ blk, const u64 *__restrict__ addr, uint32_t nb,
                                                    const BaiState *__restrict__ prev, const u64 *__restrict__ tile_base, BaiHead *__restrict__ out,
                                                    u64 n_out)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * kBaiTile;
    u64 at0 = tile_base[blockIdx.x];
    for (uint32_t k = 0; k < kBaiTile; k += kWave) {
        if (t0 + k >= n) break;
        const uint64_t i = t0 + k + threadIdx.x;
        const bool on = i < n && head[i];
        u64 total;
        const u64 at = at0 + wave_excl_scan((u64)(on ? 1 : 0), total);
        at0 += total;
        if (on && at < n_out) {
            const uint64_t o = rec_off[i];
            uint32_t w[3];                           // refID, pos, bin_mq_nl
            bai_words<3>(raw + o + 4, w);
            out[at] = BaiHead{i == 0 ? prev->last_end : bai_voffset(blk, addr, nb, o), w[2] >> 16, (int32_t)w[0]};
        }
    }
}

// One target's linear index made final: windows [0, n) with n from the target's last mapped record; a window no record reached
// takes the value to its left, window 0 the value 0.  256 windows at a time: the position of the last reached window at or
// before every window by a max-scan through LDS.
__global__ __launch_bounds__(kBaiThreads) void k_bai_fill(u64 *__restrict__ lin, const u64 *__restrict__ win_base, const u64 *__restrict__ last_mapped,
                                                          int32_t n_ref)
{
    __shared__ int32_t s_at[kBaiThreads];
    __shared__ u64 s_val[kBaiThreads];
    __shared__ u64 s_carry;
    for (int32_t t = (int32_t)blockIdx.x; t < n_ref; t += (int32_t)gridDim.x) {
        const uint32_t width = (uint32_t)(win_base[t + 1] - win_base[t]);
        uint32_t n = (uint32_t)(last_mapped[t] & 0xfffffu);
        if (n > width) n = width;                    // (inside the domain it never is)
        u64 *row = lin + win_base[t];
        if (threadIdx.x == 0) s_carry = 0;
        __syncthreads();
        for (uint32_t j0 = 0; j0 < n; j0 += kBaiThreads) {
            const uint32_t j = j0 + threadIdx.x;
            const u64 v = j < n ? row[j] : kBaiEmpty;
            s_val[threadIdx.x] = v;
            s_at[threadIdx.x] = v != kBaiEmpty ? (int32_t)threadIdx.x : -1;
            __syncthreads();
            for (int d = 1; d < kBaiThreads; d *= 2) {
                const int32_t mine = s_at[threadIdx.x], left = (int)threadIdx.x >= d ? s_at[threadIdx.x - d] : -1;
                __syncthreads();
                s_at[threadIdx.x] = left > mine ? left : mine;
                __syncthreads();
            }
            const int32_t src = s_at[threadIdx.x];
            const u64 filled = src >= 0 ? s_val[src] : s_carry;
            if (j < n) row[j] = filled;
            __syncthreads();
            if (threadIdx.x == kBaiThreads - 1) s_carry = filled;
            __syncthreads();
        }
    }
}

static inline unsigned bai_grid(uint64_t n) { return (unsigned)((n + kBaiThreads - 1) / kBaiThreads); }

uint32_t bai_tiles(uint64_t n) { return (uint32_t)((n + kBaiTile - 1) / kBaiTile); }

hipError_t launch_bai_records(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, int32_t n_ref, uint64_t base, const void *blk, const u64 *addr,
                              uint32_t nb, const int32_t *target_len, const u64 *win_base, const void *prev, void *next, uint8_t *head, u64 *counts,
                              u64 *last_mapped, u64 *lin, u64 *tile_sum, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_bai_records, dim3(bai_grid(n)), dim3(kBaiThreads), 0, st, raw, rec_off, n, n_ref, base, (const BaiBlock *)blk, addr, nb,
                       target_len, win_base, (const BaiState *)prev, (BaiState *)next, head, counts, last_mapped, lin, info);
    const uint32_t tiles = bai_tiles(n);
    hipLaunchKernelGGL(k_bai_count, dim3(tiles), dim3(kBaiThreads), 0, st, head, n, tile_sum);
    hipLaunchKernelGGL(k_bai_tiles, dim3(1), dim3(1024), 0, st, tile_sum, tiles, info);
    return hipGetLastError();
}

hipError_t launch_bai_emit(const uint8_t *raw, const uint64_t *rec_off, const uint8_t *head, uint64_t n, const void *blk, const u64 *addr, uint32_t nb,
                           const void *prev, const u64 *tile_base, void *out, uint64_t n_out, hipStream_t st)
{
    if (!n || !n_out) return hipSuccess;
    hipLaunchKernelGGL(k_bai_emit, dim3(bai_tiles(n)), dim3(kWave), 0, st, raw, rec_off, head, n, (const BaiBlock *)blk, addr, nb,
                       (const BaiState *)prev, tile_base, (BaiHead *)out, (u64)n_out);
    return hipGetLastError();
}

hipError_t launch_bai_fill(u64 *lin, const u64 *win_base, const u64 *last_mapped, int32_t n_ref, hipStream_t st)
{
    if (n_ref <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bai_fill, dim3((unsigned)(n_ref < 4096 ? n_ref : 4096)), dim3(kBaiThreads), 0, st, lin, win_base, last_mapped, n_ref);
    return hipGetLastError();
}

}  // namespace hpn
