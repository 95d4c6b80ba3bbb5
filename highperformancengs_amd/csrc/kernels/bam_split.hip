// bam_split.hip -- bamSplitChr on the device: where a coordinate-sorted BAM's records change target, whether the file lies
// in the tool's domain, where samtools' writer would cut each target's records into BGZF blocks, and -- for uncompressed
// output -- the finished blocks themselves.  (docs/kernels/bam_split.md)
//
// Within the domain a target's records are ONE slice of the inflated stream, so nothing is scattered: the kernels find
// boundaries and cuts, the bytes stay where they are.  A batch is seen as m = n + 1 items: item 0 is the target's block
// the batch before left open (its `fill` bytes lie in front of the records in the payload buffer; a size of 0 when there is
// none), items 1..n are the batch's records.  Q[i] is where item i starts in the payload buffer, Q[m] its end.
//
//   k_split_keys    per record: refID, pos, size read in place (rec_off[] of hpn_bam_raw_index_dev); order against the
//                   record before (the batch's first against the state carried from the batch before), ranges; the lowest
//                   offending ordinal through one atomicMin; where refID changes, the two targets' record counts move
//   k_split_next    per item: the item at whose start the NEXT block opens if a block opens at this one's start
//                   (bam_write1's bgzf_flush_try + bgzf_write, bgzf.c: close when off + s > 0xff00, close at once at
//                   0xff00) -- two binary searches, no chain
//   k_split_double  pointer doubling from item 0: after round k every item within 2^(k+1) hops of it is marked
//   k_split_count / k_split_tiles / k_split_emit   blocks per marked item, their exclusive scan, the block list
//   k_split_stored  level 0: every closed block as BGZF header + one stored deflate block + CRC-32 + ISIZE
#include "common.hpp"
#include "scan.hpp"

namespace hpn {

constexpr uint32_t kBgzfFull = 0xff00;          // BGZF_BLOCK_SIZE (bgzf.c:41): what a block holds before it is closed
constexpr int kSplitThreads = 256;
#ifdef HPN_TEST_HOOKS
constexpr uint32_t kSplitTile = 64;             // (the test-hooks build: a batch of 70,000 records is more than 1,024 tiles)
#else
constexpr uint32_t kSplitTile = 4096;           // items per workgroup in the scan of the block counts
#endif

struct SplitBlock {      // hpn_split_block
    uint64_t off;
    uint32_t len, crc;
    int32_t tid;
    uint32_t reserved;
};

struct SplitState {      // carried from batch to batch on the device (two of them, used in turn)
    int32_t tid, pos;
    uint32_t have, pad;
};

// info (u64 words): [0] lowest (ordinal << 3 | reason), ~0 none   [1] stream offset of the batch's first record
//                   [2] stream offset behind its last record       [3] blocks the batch makes (k_split_tiles)
__global__ __launch_bounds__(kSplitThreads) void k_split_keys(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off,
                                                              uint64_t n, int32_t n_ref, uint64_t base, uint32_t fill, uint32_t open_key,
                                                              const SplitState *__restrict__ prev, SplitState *__restrict__ next,
                                                              u64 *__restrict__ Q, uint32_t *__restrict__ key, u64 *__restrict__ counts,
                                                              u64 *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (i == 0) {
        Q[0] = 0, key[0] = open_key;
        if (n == 0) {
            Q[1] = fill;
            *next = *prev;
        }
    }
    if (i >= n) return;
    const uint64_t first = rec_off[0], o = rec_off[i];
    int32_t f[3];                                    // block_size, refID, pos (records are not aligned: bytes)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint8_t *q = raw + o + 4 * k;
        f[k] = (int32_t)((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
    }
    const int32_t tid = f[1], pos = f[2];
    int32_t ptid, ppos;
    bool have;
    if (i == 0) {
        ptid = prev->tid, ppos = prev->pos, have = prev->have != 0;
    } else {
        const uint8_t *q = raw + rec_off[i - 1] + 4;
        ptid = (int32_t)((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
        ppos = (int32_t)((uint32_t)q[4] | (uint32_t)q[5] << 8 | (uint32_t)q[6] << 16 | (uint32_t)q[7] << 24);
        have = true;
    }
    uint32_t reason = 0;
    if (tid < -1 || tid >= n_ref) reason = 1;                                    // refID outside the header's targets
    else if (tid >= 0 && (pos < 0 || pos >= (1 << 29))) reason = 2;              // a placed record without a position bam_fetch reaches
    else if (have && (uint32_t)tid < (uint32_t)ptid) reason = 3;                 // refID goes backwards (-1 sorts last)
    else if (have && tid == ptid && tid >= 0 && pos < ppos) reason = 4;          // pos goes backwards inside a target
    if (reason) atomicMin(&info[0], (u64)((base + i) << 3 | reason));
    Q[i + 1] = (u64)fill + (o - first);
    key[i + 1] = (uint32_t)tid;
    // record counts: a target's records are the ordinals between two changes of refID
    const bool in = tid >= 0 && tid < n_ref, pin = have && ptid >= 0 && ptid < n_ref;
    if (!have || tid != ptid) {
        if (in) atomicAdd(&counts[tid], (u64)0 - (u64)i);
        if (i != 0 && pin) atomicAdd(&counts[ptid], (u64)i);
    }
    if (i == 0) info[1] = first;
    if (i == n - 1) {
        if (in) atomicAdd(&counts[tid], (u64)n);
        const uint64_t end = o + 4 + (uint64_t)(uint32_t)f[0];
        info[2] = end;
        Q[n + 1] = (u64)fill + (end - first);
        next->tid = tid, next->pos = pos, next->have = 1u, next->pad = 0u;
    }
}

// first j in [lo, m) with Q[j + 1] - from > 0xff00, else m  (Q ascends)
__device__ __forceinline__ uint64_t split_first_over(const u64 *__restrict__ Q, uint64_t lo, uint64_t m, u64 from)
{
    uint64_t hi = m;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (Q[mid + 1] - from > kBgzfFull) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Where the next block opens if one opens at the start of item i, and how many blocks item i's own block run is.
// An item of s <= 0xff00 bytes opens one block that takes the items behind it while they fit (an exact fill closes it, which
// is the same cut).  A longer one is written through: s / 0xff00 full blocks, and the rest stays open for what follows.
// The block ends with the target in any case.  Items of no target (refID -1, item 0 without an open block) make no block.
__global__ __launch_bounds__(kSplitThreads) void k_split_next(const u64 *__restrict__ Q, const uint32_t *__restrict__ key, uint64_t m,
                                                              int32_t n_ref, uint32_t *__restrict__ next, uint32_t *__restrict__ mark)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (i > m) return;
    mark[i] = i == 0 ? 1u : 0u;
    if (i == m) {
        next[m] = (uint32_t)m;
        return;
    }
    const uint32_t k = key[i];
    uint64_t e = i + 1;                              // first item of another target behind i (keys ascend inside the domain)
    if (e < m && key[e] == k) {
        uint64_t lo = e + 1, hi = m;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (key[mid] > k) hi = mid;
            else lo = mid + 1;
        }
        e = lo;
    }
    uint64_t j = e;
    if (k < (uint32_t)n_ref) {
        const u64 at = Q[i], s = Q[i + 1] - at;
        if (s <= kBgzfFull) j = split_first_over(Q, i + 1, m, at);
        else if (s % kBgzfFull == 0) j = i + 1;
        else j = split_first_over(Q, i + 1, m, at + s / kBgzfFull * kBgzfFull);
        if (j > e) j = e;
    }
    next[i] = (uint32_t)j;
}

__global__ __launch_bounds__(kSplitThreads) void k_split_double(const uint32_t *__restrict__ jump, uint32_t *__restrict__ jump2,
                                                                uint32_t *__restrict__ mark, uint64_t m)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (i > m) return;
    const uint32_t j = jump[i];
    if (mark[i]) mark[j] = 1u;                       // (a mark seen early is a true one: only items on the chain are ever marked)
    jump2[i] = jump[j];
}

// blocks a marked item makes: its full blocks and the block that ends where the next one opens (none of no bytes)
__device__ __forceinline__ uint32_t split_blocks_of(const u64 *__restrict__ Q, const uint32_t *__restrict__ key, const uint32_t *__restrict__ next,
                                                    int32_t n_ref, uint64_t i)
{
    if (key[i] >= (uint32_t)n_ref) return 0;
    const u64 at = Q[i], s = Q[i + 1] - at, end = Q[next[i]];
    if (s <= kBgzfFull) return end > at ? 1u : 0u;
    const u64 full = s / kBgzfFull;
    return (uint32_t)full + (end > at + full * kBgzfFull ? 1u : 0u);
}

// tile_sum[t] = blocks of the marked items of tile t
__global__ __launch_bounds__(kSplitThreads) void k_split_count(const u64 *__restrict__ Q, const uint32_t *__restrict__ key,
                                                               const uint32_t *__restrict__ next, const uint32_t *__restrict__ mark, uint64_t m,
                                                               int32_t n_ref, u64 *__restrict__ tile_sum)
{
    __shared__ uint32_t part[kSplitThreads / kWave];
    const uint64_t t0 = (uint64_t)blockIdx.x * kSplitTile;
    uint32_t mine = 0;
    for (uint32_t k = threadIdx.x; k < kSplitTile; k += kSplitThreads) {
        const uint64_t i = t0 + k;
        if (i < m && mark[i]) mine += split_blocks_of(Q, key, next, n_ref, i);
    }
    mine = wave_sum(mine);
    if (lane_id() == 0) part[wave_id()] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int w = 0; w < kSplitThreads / kWave; ++w) s += part[w];
        tile_sum[blockIdx.x] = s;
    }
}

// exclusive scan of the tile sums in place (one workgroup; a batch of 10^7 records has ~2,500 tiles), the total into info[3]
__global__ __launch_bounds__(1024) void k_split_tiles(u64 *__restrict__ tile_sum, uint32_t n_tiles, u64 *__restrict__ info)
{
    __shared__ u64 part[1024];
    const uint32_t per = (n_tiles + 1023) / 1024, a = threadIdx.x * per, b = a + per < n_tiles ? a + per : n_tiles;
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
        info[3] = run;
    }
    __syncthreads();
    u64 run = part[threadIdx.x];
    for (uint32_t t = a; t < b; ++t) {
        const u64 v = tile_sum[t];
        tile_sum[t] = run, run += v;
    }
}

// the block list in file order: one wave per 64 consecutive items, the waves of a tile one after the other
__global__ __launch_bounds__(kWave) void k_split_emit(const u64 *__restrict__ Q, const uint32_t *__restrict__ key, const uint32_t *__restrict__ next,
                                                      const uint32_t *__restrict__ mark, uint64_t m, int32_t n_ref,
                                                      const u64 *__restrict__ tile_base, SplitBlock *__restrict__ out, u64 n_out)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * kSplitTile;
    u64 base = tile_base[blockIdx.x];
    for (uint32_t k = 0; k < kSplitTile; k += kWave) {
        const uint64_t i = t0 + k + threadIdx.x;
        if (t0 + k >= m) break;
        const bool on = i < m && mark[i];
        const uint32_t c = on ? split_blocks_of(Q, key, next, n_ref, i) : 0u;
        u64 total;
        u64 at = base + wave_excl_scan((u64)c, total);
        base += total;
        if (c) {
            const u64 from = Q[i], s = Q[i + 1] - from, end = Q[next[i]];
            u64 p = from;
            uint32_t left = c;
            if (s > kBgzfFull)
                for (u64 f = s / kBgzfFull; f && left; --f, --left, ++at, p += kBgzfFull)
                    if (at < n_out) out[at] = SplitBlock{p, kBgzfFull, 0u, (int32_t)key[i], 0u};
            if (left && at < n_out) out[at] = SplitBlock{p, (uint32_t)(end - p), 0u, (int32_t)key[i], 0u};
        }
    }
}

// One closed block -> its BGZF image of len + 31 bytes at img + spec.img_off (a workgroup per block): the 18-byte header with
// BSIZE, one final stored deflate block (01 LEN NLEN), the payload, CRC-32, ISIZE -- what deflate() at level 0 makes of at most
// 0xff00 bytes in one Z_FINISH call.  The payload moves in 16-byte pieces where source and destination share their residue
// mod 16 (head and tail by bytes), by bytes otherwise.  Nothing outside [img_off, img_off + len + 31) is written.
struct StoredSpec {
    uint64_t off, img_off;
    uint32_t len, crc;
};
__global__ __launch_bounds__(kSplitThreads) void k_split_stored(const uint8_t *__restrict__ pay, const StoredSpec *__restrict__ specs,
                                                                uint8_t *__restrict__ img)
{
    const StoredSpec sp = specs[blockIdx.x];
    uint8_t *dst = img + sp.img_off;
    const uint32_t len = sp.len, bsize = len + 30;          // BSIZE = total block size - 1
    if (threadIdx.x < 23) {
        const uint32_t t = threadIdx.x;
        const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
        uint8_t v;
        if (t < 18) v = head[t];
        else if (t == 18) v = 1;
        else if (t == 19) v = (uint8_t)len;
        else if (t == 20) v = (uint8_t)(len >> 8);
        else if (t == 21) v = (uint8_t)~len;
        else v = (uint8_t)(~len >> 8);
        dst[t] = v;
    } else if (threadIdx.x < 31) {
        const uint32_t t = threadIdx.x - 23;
        dst[23 + len + t] = (uint8_t)((t < 4 ? sp.crc : len) >> (8 * (t & 3)));
    }
    const uint8_t *s = pay + sp.off;
    uint8_t *d = dst + 23;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
        uint32_t head = (uint32_t)((16 - ((uintptr_t)d & 15)) & 15);
        if (head > len) head = len;
        const uint32_t vec = (len - head) / 16, tail0 = head + vec * 16;
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        const u32 *sv = (const u32 *)(s + head);
        u32 *dv = (u32 *)(d + head);
        for (uint32_t k = threadIdx.x; k < vec; k += kSplitThreads) dv[k] = load_stream16(sv + k);
        if (tail0 + threadIdx.x < len) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];      // (fewer than 16 bytes)
    } else {
        for (uint32_t k = threadIdx.x; k < len; k += kSplitThreads) d[k] = s[k];
    }
}

static inline unsigned split_grid(uint64_t n) { return (unsigned)((n + kSplitThreads - 1) / kSplitThreads); }

hipError_t launch_split_keys(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, int32_t n_ref, uint64_t base, uint32_t fill,
                             uint32_t open_key, const void *prev, void *next, u64 *Q, uint32_t *key, u64 *counts, u64 *info, hipStream_t st)
{
    hipLaunchKernelGGL(k_split_keys, dim3(n ? split_grid(n) : 1u), dim3(kSplitThreads), 0, st, raw, rec_off, n, n_ref, base, fill, open_key,
                       (const SplitState *)prev, (SplitState *)next, Q, key, counts, info);
    return hipGetLastError();
}

uint32_t split_tiles(uint64_t m) { return (uint32_t)((m + kSplitTile - 1) / kSplitTile); }

// next[] and the marks of the true chain; `a`, `b`: two arrays of m + 1 words, the chain's next[] is left in `a`.
// ceil(log2(m)) rounds of doubling: every launch is over all items, no lane follows the chain.
hipError_t launch_split_cuts(const u64 *Q, const uint32_t *key, uint64_t m, int32_t n_ref, uint32_t *a, uint32_t *b, uint32_t *c, uint32_t *mark,
                             u64 *tile_sum, u64 *info, hipStream_t st)
{
    const unsigned g = split_grid(m + 1);
    hipLaunchKernelGGL(k_split_next, dim3(g), dim3(kSplitThreads), 0, st, Q, key, m, n_ref, a, mark);
    hipError_t e = hipMemcpyAsync(b, a, (m + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
    uint32_t *from = b, *to = c;
    for (uint64_t reach = 1; reach < m; reach *= 2) {
        hipLaunchKernelGGL(k_split_double, dim3(g), dim3(kSplitThreads), 0, st, from, to, mark, m);
        uint32_t *t = from;
        from = to, to = t;
    }
    const uint32_t tiles = split_tiles(m);
    hipLaunchKernelGGL(k_split_count, dim3(tiles), dim3(kSplitThreads), 0, st, Q, key, a, mark, m, n_ref, tile_sum);
    hipLaunchKernelGGL(k_split_tiles, dim3(1), dim3(1024), 0, st, tile_sum, tiles, info);
    return hipGetLastError();
}

hipError_t launch_split_emit(const u64 *Q, const uint32_t *key, const uint32_t *next, const uint32_t *mark, uint64_t m, int32_t n_ref,
                             const u64 *tile_base, void *out, uint64_t n_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_split_emit, dim3(split_tiles(m)), dim3(kWave), 0, st, Q, key, next, mark, m, n_ref, tile_base, (SplitBlock *)out,
                       (u64)n_out);
    return hipGetLastError();
}

hipError_t launch_split_stored(const uint8_t *pay, const void *specs, uint32_t n, uint8_t *img, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_split_stored, dim3(n), dim3(kSplitThreads), 0, st, pay, (const StoredSpec *)specs, img);
    return hipGetLastError();
}

}  // namespace hpn
