// fastq_pair.hip -- gfx950 kernels of hpn_fastq_pair_* (pick_pair.c on the device).
//
// The reference walks two FASTQ files against each other, one strncmp per step on one thread:
//     loop: a = next(A); b = next(B)
//           while a && c(a, b) < 0:  a -> 1_SE; a = next(A)
//           while b && c(a, b) > 0:  b -> 2_SE; b = next(B)
//           if !a && !b: stop
//           a -> 1_PE; b -> 2_PE
// with c(a, b) = strncmp(a.name, b.name, k), k the offset of the first space in A's name.  The walk is a chain, but whether a
// PROPOSED pairing m[i] (the B ordinal of A record i, or none) is what the walk produces can be checked record by record
// (V1 .. V5, docs/kernels/fastq_pair.md): the device proposes -- the identity, or a join that takes B for ascending -- and
// verifies; what does not verify is left to the host's walk.  Both streams lie in device stores (hpn_store.hpp) with the 16-byte
// SortDesc of k_sort_frame per record.
//
//   k_pair_klen     k per A record (pair_cmp.hpp: 16-byte loads that end with the name), one lane per record.
//   k_pair_identity m[i] = i.
//   k_pair_find     the join: per A record the first B ordinal j with c(a, b_j) <= 0, searched OUTWARD from the proportional
//                   guess i * nB / nA by doubling steps, then by bisection; paired when c is 0 there.  4 lanes per record
//                   compare 64 bytes of both names per step; the first differing byte is found with a ballot.
//   k_pair_flags    flagA[i] = A record i is paired, flagB[m[i]] = 1; uniq_scan64 ranks both.
//   k_pair_scatter  the pair list (pairA[t], pairB[t]) by rank.
//   k_pair_verify   one comparison per record of either file: V2 for a paired A record (and V1 against the pair before), V3 for
//                   an unpaired one (against the first B record behind the pair before), V4 for an unpaired B record (against the
//                   A record of the next pair), V5 where no pair follows.  The smallest failing (mate << 31 | ordinal) is kept
//                   with one atomicMin.
//   k_pair_sizes    a mate's output bytes per record, in the paired or the single column; two scans give the offsets.
//   k_pair_write    k_sort_write's shape: 16 lanes per record copy name, sequence and the quality line WITH its line end (the
//                   reference keeps it: a last line without '\n' goes out without one) into the mate's _PE or _SE text.
//
// Bound: the join is latency -- dependent probes of names that are scattered over the store; everything else streams the
// descriptors once and the text once (docs/kernels/fastq_pair.md has the bytes and the expectation).
#include "pair_cmp.hpp"
#include "sort_desc.hpp"
#include "text_common.hpp"

namespace hpn {

constexpr int kPairTeamsPerWave = kWave / kPairTeam;
constexpr uint32_t kPairTeamsPerBlock = kTxtThreads / kPairTeam;

__global__ __launch_bounds__(256) void k_pair_klen(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc, uint32_t n,
                                                   uint32_t *__restrict__ klen)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const SortDesc d = desc[i];
    klen[i] = pair_klen(text + d.off, d.nlen);
}

__global__ __launch_bounds__(256) void k_pair_identity(uint32_t n, uint32_t *__restrict__ m)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) m[i] = i;
}

// c(a, b) by the lane's team; EVERY lane of the wave calls it (a team without work passes len 0).  len and tail: pair_span's.
__device__ __forceinline__ int pair_compare_team(const uint8_t *a, const uint8_t *b, uint32_t len, int tail, int lane)
{
    const int sub = lane & (kPairTeam - 1), first = lane - sub;
    int res = tail;
    bool done = false;
    for (uint32_t base = 0;; base += 16u * kPairTeam) {
        const bool act = !done && base < len;   // the same in all lanes of a team
        if (!__any(act)) break;
        bool less = false;
        const uint32_t p = act ? pair_lane_diff(a, b, len, base + 16u * (uint32_t)sub, &less) : kPairNone;
        const u64 hit = __ballot(p != kPairNone), lt = __ballot(less);
        const uint32_t mine = (uint32_t)(hit >> first) & ((1u << kPairTeam) - 1u);
        if (mine) {   // the lowest lane that saw a difference holds the first one: a moved-back piece only repeats its neighbour's bytes
            const int src = first + __builtin_ctz(mine);
            res = ((lt >> src) & 1ull) ? -1 : 1;
            done = true;
        }
    }
    return res;
}

// m[i]: the first B ordinal j with c(a_i, b_j) <= 0 if c is 0 there, else kPairNone.  "First" holds where c(a_i, b_j) > 0 is
// true up to some j and false from there on; on other inputs the search still ends inside [0, nB] and k_pair_verify decides.
__global__ __launch_bounds__(kTxtThreads) void k_pair_find(const uint8_t *__restrict__ textA, const SortDesc *__restrict__ descA,
                                                           const uint32_t *__restrict__ klen, uint32_t nA,
                                                           const uint8_t *__restrict__ textB, const SortDesc *__restrict__ descB,
                                                           uint32_t nB, uint32_t *__restrict__ m)
{
    const int lane = lane_id(), sub = lane & (kPairTeam - 1);
    for (u64 base = (u64)blockIdx.x * kPairTeamsPerBlock + (u64)wave_id() * kPairTeamsPerWave; base < nA;
         base += (u64)gridDim.x * kPairTeamsPerBlock) {
        const u64 i = base + (u64)(lane / kPairTeam);
        const bool valid = i < nA;
        SortDesc da = {0, 0, 0, 0, 0};
        uint32_t k = 0;
        if (valid) da = descA[i], k = klen[i];
        const uint8_t *a = textA + da.off;
        // P(j) = c(a, b_j) <= 0.  P(lo) is false (lo = -1: nothing), P(hi) true (hi = nB: nothing); probes lie strictly between
        long long lo = -1, hi = nB, probe = 0;
        bool fin = !valid || nB == 0u, eq = false, gallop = true;
        int dir = 0;
        long long step = 1;
        if (!fin) {
            probe = (long long)(i * (u64)nB / (u64)nA);
            if (probe > (long long)nB - 1) probe = (long long)nB - 1;
        }
        while (__any(!fin)) {
            uint32_t len = 0;
            int tail = 0;
            const uint8_t *b = textB;
            if (!fin) {
                const SortDesc db = descB[probe];
                pair_span(k, da.nlen, db.nlen, &len, &tail);
                b = textB + db.off;
            }
            const int c = pair_compare_team(a, b, len, tail, lane);
            if (fin) continue;
            const bool P = c <= 0;
            if (P) hi = probe, eq = c == 0;
            else lo = probe;
            if (dir == 0) dir = P ? -1 : 1;                        // the guess decides the direction
            else if (gallop && (dir < 0) != P) gallop = false;     // the doubling steps have passed the border
            if (hi - lo <= 1) {
                fin = true;
                continue;
            }
            long long next = lo + (hi - lo) / 2;
            if (gallop) {
                const long long cand = dir < 0 ? hi - step : lo + step;
                step <<= 1;
                if (cand > lo && cand < hi) next = cand;
                else gallop = false;
            }
            probe = next;
        }
        if (valid && sub == 0) m[i] = (hi < (long long)nB && eq) ? (uint32_t)hi : kPairNone;
    }
}

// flagB: zeroed before the launch.  m[i] < nB (k_pair_find and, with nA == nB, k_pair_identity give no other).
__global__ __launch_bounds__(256) void k_pair_flags(const uint32_t *__restrict__ m, uint32_t nA, uint32_t *__restrict__ flagA,
                                                    uint32_t *__restrict__ flagB)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nA) return;
    const uint32_t j = m[i];
    flagA[i] = j != kPairNone ? 1u : 0u;
    if (j != kPairNone) flagB[j] = 1u;
}

// rankA: the exclusive scan of flagA
__global__ __launch_bounds__(256) void k_pair_scatter(const uint32_t *__restrict__ m, const uint64_t *__restrict__ rankA, uint32_t nA,
                                                      uint32_t *__restrict__ pairA, uint32_t *__restrict__ pairB)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nA) return;
    const uint32_t j = m[i];
    if (j == kPairNone) return;
    const uint64_t t = rankA[i];
    pairA[t] = i, pairB[t] = j;
}

// One team per record: items [0, nA) are A's, [nA, nA + nB) B's.  rankA[nA] is the number of pairs.  fail: 0xffffffff before
// the launch.
__global__ __launch_bounds__(kTxtThreads) void k_pair_verify(const uint8_t *__restrict__ textA, const SortDesc *__restrict__ descA,
                                                             const uint32_t *__restrict__ klen, uint32_t nA,
                                                             const uint8_t *__restrict__ textB, const SortDesc *__restrict__ descB,
                                                             uint32_t nB, const uint32_t *__restrict__ m,
                                                             const uint64_t *__restrict__ rankA, const uint32_t *__restrict__ flagB,
                                                             const uint64_t *__restrict__ rankB, const uint32_t *__restrict__ pairA,
                                                             const uint32_t *__restrict__ pairB, uint32_t *__restrict__ fail)
{
    const int lane = lane_id(), sub = lane & (kPairTeam - 1);
    const u64 total = (u64)nA + nB, n_pairs = rankA[nA];
    for (u64 base = (u64)blockIdx.x * kPairTeamsPerBlock + (u64)wave_id() * kPairTeamsPerWave; base < total;
         base += (u64)gridDim.x * kPairTeamsPerBlock) {
        const u64 item = base + (u64)(lane / kPairTeam);
        // the one comparison c(a_ia, b_ib) and the sign it must have; bad: the record fails without one
        bool cmp = false, bad = false;
        uint32_t ia = 0, ib = 0, code = 0;
        int want = 0;
        if (item < nA) {
            ia = (uint32_t)item, code = ia;
            const uint32_t j = m[ia];
            const u64 t = rankA[ia];   // paired: its pair; else the next pair
            if (j != kPairNone) {
                if (t && pairB[t - 1u] >= j) bad = true;   // V1
                ib = j, want = 0, cmp = !bad;              // V2
            } else if (t >= n_pairs) {
                bad = true;   // V5: an A record behind the last pair
            } else {
                ib = t ? pairB[t - 1u] + 1u : 0u;   // V3: the first B record behind the pair before
                if (ib >= nB) bad = true;
                want = -1, cmp = !bad;
            }
        } else if (item < total) {
            ib = (uint32_t)(item - nA), code = 0x80000000u | ib;
            if (!flagB[ib]) {
                const u64 t = rankB[ib];   // paired B records in front of it: the next pair
                if (t >= n_pairs) bad = true;   // V5
                else ia = pairA[t], want = 1, cmp = true;   // V4
            }
        }
        uint32_t len = 0;
        int tail = 0;
        const uint8_t *a = textA, *b = textB;
        if (cmp) {
            const SortDesc da = descA[ia], db = descB[ib];
            pair_span(klen[ia], da.nlen, db.nlen, &len, &tail);
            a = textA + da.off, b = textB + db.off;
        }
        const int c = pair_compare_team(a, b, len, tail, lane);
        if (cmp && (want == 0 ? c != 0 : want < 0 ? c >= 0 : c <= 0)) bad = true;
        if (bad && sub == 0) atomicMin(fail, code);
    }
}

// flag[i]: record i is paired.  Its bytes -- "%s\n%s\n+\n%s", the quality line with its line end -- count in pe[i] or se[i].
__global__ __launch_bounds__(256) void k_pair_sizes(const SortDesc *__restrict__ desc, const uint32_t *__restrict__ flag, uint32_t n,
                                                    uint32_t *__restrict__ pe, uint32_t *__restrict__ se)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const SortDesc d = desc[i];
    const uint32_t size = (uint32_t)d.nlen + 1u + d.slen + 3u + d.qlen + 1u;
    const bool paired = flag[i] != 0u;
    pe[i] = paired ? size : 0u, se[i] = paired ? 0u : size;
}

// off_pe, off_se: the exclusive scans of k_pair_sizes' columns
__global__ __launch_bounds__(kTxtThreads) void k_pair_write(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc,
                                                            const uint32_t *__restrict__ flag, const uint64_t *__restrict__ off_pe,
                                                            const uint64_t *__restrict__ off_se, uint32_t n, uint8_t *__restrict__ out_pe,
                                                            uint8_t *__restrict__ out_se)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0;
        uint8_t *dst = nullptr;
        uint32_t nlen = 0, slen = 0, qlen = 0, qrel = 0;
        if (k < n) {
            const SortDesc d = desc[k];
            src = d.off, dst = flag[k] ? out_pe + off_pe[k] : out_se + off_se[k];
            nlen = d.nlen, slen = d.slen, qlen = d.qlen, qrel = d.qrel;
            uint8_t *o = dst + nlen;   // the fixed bytes, by the record's own lane
            o[0] = '\n';
            o += 1u + slen;
            o[0] = '\n', o[1] = '+', o[2] = '\n';
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl((u64)dst, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), cj = __shfl(slen, j, kWave), mj = __shfl(qlen, j, kWave);
            const uint32_t rj = __shfl(qrel, j, kWave);
            if (k0 + (uint32_t)j >= n) continue;
            uint8_t *o = (uint8_t *)dj;
            copy_span(text + sj, o, nj, sub);
            copy_span(text + sj + nj + 1u, o + nj + 1u, cj, sub);
            copy_span(text + sj + rj, o + nj + 1u + cj + 3u, mj + 1u, sub);   // the byte behind the quality: its '\n', or the last byte of a line without one
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned blocks256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }
static inline unsigned team_blocks(uint64_t items, int n_cu)
{
    const uint64_t want = (items + kPairTeamsPerBlock - 1) / kPairTeamsPerBlock, cap = (uint64_t)n_cu * 16;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

hipError_t launch_pair_klen(const uint8_t *d_text, const void *d_desc, uint32_t n, uint32_t *d_klen, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_pair_klen, dim3(blocks256(n)), dim3(256), 0, st, d_text, (const SortDesc *)d_desc, n, d_klen);
    return hipGetLastError();
}

hipError_t launch_pair_identity(uint32_t n, uint32_t *d_m, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_pair_identity, dim3(blocks256(n)), dim3(256), 0, st, n, d_m);
    return hipGetLastError();
}

hipError_t launch_pair_find(const uint8_t *d_text_a, const void *d_desc_a, const uint32_t *d_klen, uint32_t n_a, const uint8_t *d_text_b,
                            const void *d_desc_b, uint32_t n_b, uint32_t *d_m, int n_cu, hipStream_t st)
{
    if (!n_a) return hipSuccess;
    hipLaunchKernelGGL(k_pair_find, dim3(team_blocks(n_a, n_cu)), dim3(kTxtThreads), 0, st, d_text_a, (const SortDesc *)d_desc_a, d_klen, n_a,
                       d_text_b, (const SortDesc *)d_desc_b, n_b, d_m);
    return hipGetLastError();
}

// d_flag_b is zeroed here
hipError_t launch_pair_flags(const uint32_t *d_m, uint32_t n_a, uint32_t n_b, uint32_t *d_flag_a, uint32_t *d_flag_b, hipStream_t st)
{
    if (n_b) {
        const hipError_t e = hipMemsetAsync(d_flag_b, 0, (size_t)n_b * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    if (!n_a) return hipSuccess;
    hipLaunchKernelGGL(k_pair_flags, dim3(blocks256(n_a)), dim3(256), 0, st, d_m, n_a, d_flag_a, d_flag_b);
    return hipGetLastError();
}

hipError_t launch_pair_scatter(const uint32_t *d_m, const uint64_t *d_rank_a, uint32_t n_a, uint32_t *d_pair_a, uint32_t *d_pair_b, hipStream_t st)
{
    if (!n_a) return hipSuccess;
    hipLaunchKernelGGL(k_pair_scatter, dim3(blocks256(n_a)), dim3(256), 0, st, d_m, d_rank_a, n_a, d_pair_a, d_pair_b);
    return hipGetLastError();
}

// d_fail: set to 0xffffffff here
hipError_t launch_pair_verify(const uint8_t *d_text_a, const void *d_desc_a, const uint32_t *d_klen, uint32_t n_a, const uint8_t *d_text_b,
                              const void *d_desc_b, uint32_t n_b, const uint32_t *d_m, const uint64_t *d_rank_a, const uint32_t *d_flag_b,
                              const uint64_t *d_rank_b, const uint32_t *d_pair_a, const uint32_t *d_pair_b, uint32_t *d_fail, int n_cu,
                              hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(d_fail, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess || !((uint64_t)n_a + n_b)) return e;
    hipLaunchKernelGGL(k_pair_verify, dim3(team_blocks((uint64_t)n_a + n_b, n_cu)), dim3(kTxtThreads), 0, st, d_text_a, (const SortDesc *)d_desc_a,
                       d_klen, n_a, d_text_b, (const SortDesc *)d_desc_b, n_b, d_m, d_rank_a, d_flag_b, d_rank_b, d_pair_a, d_pair_b, d_fail);
    return hipGetLastError();
}

hipError_t launch_pair_sizes(const void *d_desc, const uint32_t *d_flag, uint32_t n, uint32_t *d_pe, uint32_t *d_se, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_pair_sizes, dim3(blocks256(n)), dim3(256), 0, st, (const SortDesc *)d_desc, d_flag, n, d_pe, d_se);
    return hipGetLastError();
}

hipError_t launch_pair_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_flag, const uint64_t *d_off_pe, const uint64_t *d_off_se,
                             uint32_t n, uint8_t *d_out_pe, uint8_t *d_out_se, int n_cu, hipStream_t st)
{
    if (!n) return hipSuccess;
    const uint64_t want = ((uint64_t)n + kTxtThreads - 1) / kTxtThreads, cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_pair_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc, d_flag,
                       d_off_pe, d_off_se, n, d_out_pe, d_out_se);
    return hipGetLastError();
}

}  // namespace hpn
