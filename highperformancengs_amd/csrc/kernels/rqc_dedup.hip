// rqc_dedup.hip -- gfx950 kernels of hpn_rfastqc_* (the R plugin's qsort_hash_count, Rgzfastq_uniq.c, on the device).
//
// The plugin keys a chained hash table by a string it assembles per record or pair (kernels/rqc_key.hpp: at most two spans, at
// most 150 bytes), counts every key, and returns the counts sorted descending beside the per-read GC fraction and the Quality /
// Nucleotide / Length tallies.  Only the multiset of counts can be seen from outside, so there is no table here: the records are
// sorted stably by a 64-bit hash of their key (radix_sort.hpp), group starts are flagged by comparing BYTES, the counts are the
// differences of the starts, and one more radix sort orders them.
//
//   k_rqc_sizes     per record: sequence and quality lengths as 32-bit sizes for the scans, Length[] in LDS, the smallest record
//                   outside the plugin's domain (L outside 1..300, a quality line beyond 300) by atomicMin, and whether any
//                   quality line's length differs from its sequence's.
//   k_rqc_gather    16 lanes per record (copy_span's pieces): sequence and quality lines from the store into the two
//                   structure-of-arrays buffers k_tally_hist and k_read_gc take; every byte is OR-ed on its way, a record with
//                   bit 7 set anywhere is reported by atomicMin.
//   k_rqc_key       16 lanes per record, four records per wave-instruction: lane s folds bytes [16 s, 16 s + 16) of the key
//                   (key_piece: one unaligned 16-byte load inside a span, bytewise at the seam and at the key's end -- never a
//                   byte outside the spans), weights its piece by the base's power and the team sums by four shuffles.  The hash
//                   is of the key's bytes alone, so the same bytes cut at another place hash alike.
//   k_rqc_flags     over the order sorted by hash: a record opens a group iff its hash, its key length or its key bytes differ
//                   from its predecessor's (the same pieces, compared by the team); equal hashes over different keys are
//                   counted, and the host then orders such runs by their bytes (hpn_rqcfile.hip).
//   k_rqc_starts / k_rqc_count_key   group starts from the flags' scan; count = next start - start, sort key = n - count.
//   k_rqc_matrices  k_tally_hist's 64-bit [row][512] matrices into the plugin's int Quality[q + 128 pos], Nucleotide[5 pos + c].
//
// Bound: HBM.  key reads 32 B of descriptors and the key's bytes per pair and writes 13 B; flags reads 12 B per position and, where
// the hashes are equal, two keys through the sorted order (scattered lines).  docs/kernels/rqc_dedup.md.
#include "rqc_key.hpp"
#include "text_common.hpp"

namespace hpn {

struct RqcView {
    const uint8_t *text[2];
    const SortDesc *desc[2];
    int paired;
};

constexpr u64 kRqcBase = 0x9E3779B97F4A7C15ull;   // odd
static_assert(2 * kRqcWhole <= 16 * 16, "a key is one piece per lane of a 16-lane team");

__device__ __forceinline__ u64 rqc_pow(uint32_t e)   // e < 256
{
    u64 r = 1u, b = kRqcBase;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (e & (1u << k)) r *= b;
        b *= b;
    }
    return r;
}

// A key as its team sees it: where its two spans start, and their lengths.
struct RqcKeyAt {
    const uint8_t *s0, *s1;
    uint32_t n0, n1;
};

// Bytes [idx, idx + 16) of the key s0[0:n0] + s1[0:n1], zeros behind its end.  A piece inside one span is one unaligned 16-byte
// load; the piece across the seam and the key's last, partial piece are assembled from byte loads.
__device__ __forceinline__ u32 key_piece(const RqcKeyAt &k, uint32_t idx)
{
    u32 w = {0u, 0u, 0u, 0u};
    const uint32_t K = k.n0 + k.n1;
    if (idx + 16u <= k.n0) {
        __builtin_memcpy(&w, k.s0 + idx, 16);
    } else if (idx >= k.n0 && idx + 16u <= K) {
        __builtin_memcpy(&w, k.s1 + (idx - k.n0), 16);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint32_t at = idx + i;
            if (at < K) w[i >> 2] |= (uint32_t)(at < k.n0 ? k.s0[at] : k.s1[at - k.n0]) << (8u * (i & 3u));
        }
    }
    return w;
}

// the descriptors of record r -> its key
__device__ __forceinline__ RqcKeyAt key_of(const RqcView &v, uint32_t r)
{
    RqcKeyAt k;
    const SortDesc a = v.desc[0][r];
    uint32_t L2 = 0;
    k.s0 = v.text[0] + a.off + a.nlen + 1u, k.s1 = nullptr;
    if (v.paired) {
        const SortDesc b = v.desc[1][r];
        k.s1 = v.text[1] + b.off + b.nlen + 1u, L2 = b.slen;
    }
    rqc_key_spans(a.slen, L2, v.paired, k.n0, k.n1);
    return k;
}

__device__ __forceinline__ RqcKeyAt key_from_lane(const RqcKeyAt &k, int j)
{
    RqcKeyAt t;
    t.s0 = (const uint8_t *)__shfl((u64)k.s0, j, kWave), t.s1 = (const uint8_t *)__shfl((u64)k.s1, j, kWave);
    t.n0 = __shfl(k.n0, j, kWave), t.n1 = __shfl(k.n1, j, kWave);
    return t;
}

// info[0]: the smallest 2 * record + mate outside the domain; info[1]: set when a quality line's length is not its sequence's
__global__ __launch_bounds__(256) void k_rqc_sizes(const SortDesc *__restrict__ desc, uint32_t n, uint32_t mate, uint32_t *__restrict__ ssz,
                                                   uint32_t *__restrict__ qsz, uint32_t *__restrict__ length, uint32_t *__restrict__ info)
{
    __shared__ uint32_t lh[kRqcMaxLen];
    for (uint32_t i = threadIdx.x; i < kRqcMaxLen; i += 256u) lh[i] = 0;
    __syncthreads();
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n) {
        const SortDesc d = desc[r];
        ssz[r] = d.slen, qsz[r] = d.qlen;
        if (d.slen < 1u || d.slen > kRqcMaxLen || d.qlen > kRqcMaxLen) atomicMin(&info[0], 2u * r + mate);
        else atomicAdd(&lh[d.slen - 1u], 1u);
        if (d.qlen != d.slen) atomicOr(&info[1], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kRqcMaxLen; i += 256u)
        if (lh[i]) atomicAdd(&length[i], lh[i]);
}

// copy_span, and the OR of what it moved
__device__ __forceinline__ uint32_t copy_span_or(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t cnt, int sub)
{
    uint32_t seen = 0;
    if (cnt >= 16u) {
        for (uint32_t i = 16u * (uint32_t)sub; i < cnt; i += 256u) {
            const uint32_t o = min(i, cnt - 16u);
            u32 v;
            __builtin_memcpy(&v, src + o, 16);
            __builtin_memcpy(dst + o, &v, 16);
            seen |= v[0] | v[1] | v[2] | v[3];
        }
    } else if ((uint32_t)sub < cnt) {
        seen = dst[sub] = src[sub];
    }
    return seen;
}

__global__ __launch_bounds__(kTxtThreads) void k_rqc_gather(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc, uint32_t n,
                                                            uint32_t mate, const uint64_t *__restrict__ soff, const uint64_t *__restrict__ qoff,
                                                            uint8_t *__restrict__ seq, uint8_t *__restrict__ qual, uint32_t *__restrict__ info)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, sdst = 0, qdst = 0;
        uint32_t nlen = 0, slen = 0, qlen = 0, qrel = 0;
        if (k < n) {
            const SortDesc d = desc[k];
            src = d.off, sdst = soff[k], qdst = qoff[k];
            nlen = d.nlen, slen = d.slen, qlen = d.qlen, qrel = d.qrel;
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dsj = __shfl(sdst, j, kWave), dqj = __shfl(qdst, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), cj = __shfl(slen, j, kWave), mj = __shfl(qlen, j, kWave), rj = __shfl(qrel, j, kWave);
            if (k0 + (uint32_t)j >= n) continue;
            const uint32_t seen = copy_span_or(text + sj + nj + 1u, seq + dsj, cj, sub) | copy_span_or(text + sj + rj, qual + dqj, mj, sub);
            if (seen & 0x80808080u) atomicMin(&info[0], 2u * (k0 + (uint32_t)j) + mate);
        }
    }
}

__global__ __launch_bounds__(kTxtThreads) void k_rqc_key(RqcView v, uint32_t n, u64 hash_mask, uint64_t *__restrict__ hash,
                                                         uint32_t *__restrict__ order, uint8_t *__restrict__ klen)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t r0 = wave * kWave; r0 < n; r0 += nwaves * kWave) {
        const uint32_t r = r0 + lane;
        RqcKeyAt mine = {nullptr, nullptr, 0u, 0u};
        if (r < n) mine = key_of(v, r);
        u64 my_h = 0;
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {   // four records per wave-instruction, 16 lanes each
            if (r0 + 4u * (uint32_t)it >= n) break;
            const RqcKeyAt k = key_from_lane(mine, 4 * it + grp);
            const uint32_t K = k.n0 + k.n1, idx = 16u * (uint32_t)sub;
            u64 h = 0;
            if (idx < K) {
                const u32 w = key_piece(k, idx);
                const uint32_t cnt = K - idx < 16u ? K - idx : 16u;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((uint32_t)i < cnt) h = h * kRqcBase + ((w[i >> 2] >> (8 * (i & 3))) & 255u);
                h *= rqc_pow(K - idx - cnt);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) h += __shfl_xor(h, o, 16);
            h += rqc_pow(K);   // the length's seed
            const u64 hh = __shfl(h, (lane & 3) * 16, kWave);   // to the record's own lane
            if ((lane >> 2) == it) my_h = hh;
        }
        if (r < n) hash[r] = my_h & hash_mask, order[r] = r, klen[r] = (uint8_t)(mine.n0 + mine.n1);
    }
}

// info[2]: records whose hash equals their predecessor's while their key differs
__global__ __launch_bounds__(kTxtThreads) void k_rqc_flags(RqcView v, const uint64_t *__restrict__ hash, const uint32_t *__restrict__ order,
                                                           const uint8_t *__restrict__ klen, uint32_t n, uint32_t *__restrict__ flag,
                                                           uint32_t *__restrict__ info)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t p0 = wave * kWave; p0 < n; p0 += nwaves * kWave) {
        const uint32_t p = p0 + lane;
        RqcKeyAt a = {nullptr, nullptr, 0u, 0u}, b = a;
        bool cmp = false, same_hash = false;
        if (p < n && p && hash[p] == hash[p - 1u]) {
            const uint32_t ra = order[p - 1u], rb = order[p];
            same_hash = true;
            if (klen[ra] == klen[rb]) cmp = true, a = key_of(v, ra), b = key_of(v, rb);
        }
        const u64 want = __ballot(cmp);
        uint32_t differs = 0;
        for (int it = 0; it < kWave / 4; ++it) {
            if (!((want >> (4 * it)) & 0xfull)) continue;   // (uniform) none of these four positions compares bytes
            const int j = 4 * it + grp;
            const RqcKeyAt ka = key_from_lane(a, j), kb = key_from_lane(b, j);
            const uint32_t K = ka.n0 + ka.n1, idx = 16u * (uint32_t)sub;
            bool d = false;
            if (((want >> j) & 1ull) && idx < K) {
                const u32 x = key_piece(ka, idx), y = key_piece(kb, idx);
                d = x[0] != y[0] || x[1] != y[1] || x[2] != y[2] || x[3] != y[3];
            }
            const u64 any = __ballot(d);
            if ((lane >> 2) == it) differs = ((any >> (16 * (lane & 3))) & 0xffffull) ? 1u : 0u;
        }
        uint32_t clash = 0;
        if (p < n) {
            const uint32_t f = !same_hash || !cmp || differs ? 1u : 0u;
            flag[p] = f;
            clash = same_hash ? f : 0u;
        }
        const uint32_t c = wave_sum(clash);
        if (lane == 0 && c) atomicAdd(&info[2], c);
    }
}

// start[g]: where group g opens in the sorted order (gid: the flags' exclusive scan); start[n_groups] = n
__global__ __launch_bounds__(256) void k_rqc_starts(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ gid, uint32_t n,
                                                    uint32_t n_groups, uint32_t *__restrict__ start)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n && flag[p]) start[gid[p]] = p;
    if (p == 0) start[n_groups] = n;
}

// ascending n - count is descending count; the payload is the count itself, which is what the sorted vector holds
__global__ __launch_bounds__(256) void k_rqc_count_key(const uint32_t *__restrict__ start, uint32_t n, uint32_t n_groups,
                                                       uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t c = start[g + 1u] - start[g];
    key[g] = n - c, val[g] = c;
}

__global__ __launch_bounds__(256) void k_rqc_matrices(const u64 *__restrict__ acc, int32_t *__restrict__ quality, int32_t *__restrict__ nucleotide)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < (uint32_t)HPN_QUAL_ROWS * kRqcMaxLen) quality[i] = (int32_t)acc[HPN_TALLY_W_QUAL + (i % HPN_QUAL_ROWS) * HPN_LEN_BINS + i / HPN_QUAL_ROWS];
    if (i < (uint32_t)HPN_NUC_CODES * kRqcMaxLen) nucleotide[i] = (int32_t)acc[HPN_TALLY_W_NUC + (i % HPN_NUC_CODES) * HPN_LEN_BINS + i / HPN_NUC_CODES];
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned blocks256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }
static inline unsigned team_blocks(uint32_t n, int n_cu)
{
    const uint64_t want = ((uint64_t)n + kTxtThreads - 1) / kTxtThreads, cap = (uint64_t)n_cu * 8;
    return (unsigned)(want < cap ? want : cap);
}

static RqcView make_view(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired)
{
    RqcView v;
    v.text[0] = t0, v.text[1] = t1, v.desc[0] = (const SortDesc *)d0, v.desc[1] = (const SortDesc *)d1, v.paired = paired;
    return v;
}

hipError_t launch_rqc_sizes(const void *d_desc, uint32_t n, uint32_t mate, uint32_t *d_ssz, uint32_t *d_qsz, uint32_t *d_length, uint32_t *d_info,
                            hipStream_t st)
{
    hipLaunchKernelGGL(k_rqc_sizes, dim3(blocks256(n)), dim3(256), 0, st, (const SortDesc *)d_desc, n, mate, d_ssz, d_qsz, d_length, d_info);
    return hipGetLastError();
}

hipError_t launch_rqc_gather(const uint8_t *d_text, const void *d_desc, uint32_t n, uint32_t mate, const uint64_t *d_soff, const uint64_t *d_qoff,
                             uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_info, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rqc_gather, dim3(team_blocks(n, n_cu)), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc, n, mate, d_soff, d_qoff,
                       d_seq, d_qual, d_info);
    return hipGetLastError();
}

hipError_t launch_rqc_key(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, uint32_t n, uint64_t hash_mask,
                          uint64_t *d_hash, uint32_t *d_order, uint8_t *d_klen, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rqc_key, dim3(team_blocks(n, n_cu)), dim3(kTxtThreads), 0, st, make_view(t0, d0, t1, d1, paired), n, (u64)hash_mask, d_hash,
                       d_order, d_klen);
    return hipGetLastError();
}

hipError_t launch_rqc_flags(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint64_t *d_hash,
                            const uint32_t *d_order, const uint8_t *d_klen, uint32_t n, uint32_t *d_flag, uint32_t *d_info, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rqc_flags, dim3(team_blocks(n, n_cu)), dim3(kTxtThreads), 0, st, make_view(t0, d0, t1, d1, paired), d_hash, d_order, d_klen,
                       n, d_flag, d_info);
    return hipGetLastError();
}

hipError_t launch_rqc_counts(const uint32_t *d_flag, const uint32_t *d_gid, uint32_t n, uint32_t n_groups, uint32_t *d_start, uint64_t *d_key,
                             uint32_t *d_val, hipStream_t st)
{
    hipLaunchKernelGGL(k_rqc_starts, dim3(blocks256(n)), dim3(256), 0, st, d_flag, d_gid, n, n_groups, d_start);
    hipLaunchKernelGGL(k_rqc_count_key, dim3(blocks256(n_groups)), dim3(256), 0, st, d_start, n, n_groups, d_key, d_val);
    return hipGetLastError();
}

hipError_t launch_rqc_matrices(const uint64_t *d_acc, int32_t *d_quality, int32_t *d_nucleotide, hipStream_t st)
{
    hipLaunchKernelGGL(k_rqc_matrices, dim3(blocks256((uint32_t)HPN_QUAL_ROWS * kRqcMaxLen)), dim3(256), 0, st, (const u64 *)d_acc, d_quality,
                       d_nucleotide);
    return hipGetLastError();
}

}  // namespace hpn
