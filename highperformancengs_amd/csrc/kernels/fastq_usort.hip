// fastq_usort.hip -- gfx950 kernels of hpn_fastq_usort_* (gzfastq_uniq_sort.c on the device).
//
// The reference keys a chained table (hashtbl.c) of S = (size_t)(1.34 * e) slots by the sequence (pairs: both sequences joined),
// new keys at the head of their chain, and never resizes it; it keeps the FIRST record of a key as its representative and
// counts the others.  dump_hash_table walks slot 0 .. S - 1, every chain head to tail, and glibc's stable qsort orders that
// array by count descending: the keys come ascending in (-count, djb2_64(key) % S, -(ordinal of the key's first record)).
// A sequence line is key[0, strLen) for mate 1 and key[strLen, end) for mate 2, strLen = the length of the first mate-1
// sequence that is not empty (gzfastq_uniq_sort.c:129) -- with reads of mixed lengths a line crosses from one mate's
// sequence into the other's.
//
// The grouping stage is gzfastq_uniq's (hpn_uniq_group.hpp): first[g] is the first record of group g, rank[first[g]] the
// group's rank by first occurrence, count[g] its records.
//
//   k_usort_seqlen   per record: the least ordinal whose mate-1 sequence is not empty (atomicMin).
//   k_usort_djb64    16 lanes per GROUP: the first record's sequence(s) folded in 16-byte words with powers of 33 modulo 2^64;
//                    the seed enters as 5381 * 33^L, a pair is H(s1) * 33^len2 + H0(s2).
//   k_usort_bucket   per group: hash % S as the sort key, laid out by DESCENDING rank of first occurrence, so that a stable
//                    sort by slot leaves every chain head to tail; the greatest count; keys the reference cannot hold.
//   k_usort_count_key   the second stable sort's key: 0xffffffff - count of the group at each position of the walk.
//   k_usort_sizes    per output position and mate: the record's bytes (a 64-bit scan gives the offsets: an output can pass 4 GiB).
//   k_usort_write    16 lanes per output record: name, '\t', decimal count, the sequence line as up to two spans, "\n+\n",
//                    quality (copy_span).
//
// Bound: HBM.  seqlen reads 32 B per record; djb64 reads per group one descriptor per mate and its sequence(s) once and writes
// 8 B; bucket reads 20 B and writes 12 B per group; sizes reads one descriptor (pairs: two) and writes 8 B per group; write
// reads and writes every kept record once.
#include "text_common.hpp"
#include "uniq_desc.hpp"

namespace hpn {

// words of the session's info block (hpn_uniq_group.hpp: kUi*; the grouping stage uses 0 .. 7)
enum { kUsMaxCount = 7, kUsFirstSeq = 8, kUsSeqLen = 9, kUsShortKey = 10, kUsLongKey = 11 };

struct UsortView {
    const uint8_t *text[2];
    const UniqDesc *desc[2];
    int paired;
};

__device__ __forceinline__ u64 pow33w(uint32_t e)   // 33^e modulo 2^64, e < 4096
{
    u64 r = 1u, b = 33u;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (e & (1u << k)) r *= b;
        b *= b;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_usort_seqlen(const UniqDesc *__restrict__ desc, uint32_t n, uint32_t *__restrict__ info)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t m = wave_max(i < n && desc[i].slen ? 0xffffffffu - i : 0u);   // the wave's least such ordinal: one atomic per wave
    if (lane_id() == 0 && m) atomicMin(&info[kUsFirstSeq], 0xffffffffu - m);
}

// sum of c[i] * 33^(len - 1 - i) over a sequence, one 16-lane team: lane `sub` holds its share, the team's sum is the whole
__device__ __forceinline__ u64 fold33(const uint8_t *__restrict__ s, uint32_t len, int sub)
{
    u64 h = 0;
    for (uint32_t o = 16u * (uint32_t)sub; o < len; o += 256u) {
        u32 w;
        __builtin_memcpy(&w, s + o, 16);   // (up to 15 bytes beyond the sequence: inside the record)
        const uint32_t cnt = len - o < 16u ? len - o : 16u;
        u64 hw = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 255u;
            if ((uint32_t)i < cnt) hw = hw * 33u + c;
        }
        h += hw * pow33w(len - o - cnt);
    }
    return h;
}

__global__ __launch_bounds__(256) void k_usort_djb64(UsortView v, const uint32_t *__restrict__ first, uint32_t n_groups,
                                                     uint64_t *__restrict__ hash)
{
    const uint32_t g = blockIdx.x * 16u + (threadIdx.x >> 4);
    const int sub = (int)(threadIdx.x & 15u);
    const bool have = g < n_groups;
    uint32_t l0 = 0, l1 = 0;
    const uint8_t *s0 = v.text[0], *s1 = v.text[0];
    if (have) {
        const uint32_t r = first[g];
        const UniqDesc a = v.desc[0][r];
        s0 = v.text[0] + a.off + a.nlen + 1u, l0 = a.slen;
        if (v.paired) {
            const UniqDesc b = v.desc[1][r];
            s1 = v.text[1] + b.off + b.nlen + 1u, l1 = b.slen;
        }
    }
    u64 h0 = fold33(s0, l0, sub), h1 = fold33(s1, l1, sub);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        h0 += __shfl_xor(h0, o, 16);
        h1 += __shfl_xor(h1, o, 16);
    }
    if (have && sub == 0) hash[g] = (5381ull * pow33w(l0) + h0) * pow33w(l1) + h1;
}

// Position U - 1 - j of the arrays belongs to the group of rank j: descending first ordinal.  Lane 0 of the grid also leaves
// strLen in info[kUsSeqLen].
__global__ __launch_bounds__(256) void k_usort_bucket(UsortView v, const uint32_t *__restrict__ first, const uint32_t *__restrict__ rank,
                                                      const uint32_t *__restrict__ count, const uint64_t *__restrict__ hash,
                                                      uint32_t n_groups, u64 table_size, uint64_t *__restrict__ key,
                                                      uint32_t *__restrict__ val, uint32_t *__restrict__ info)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t r0 = info[kUsFirstSeq];
    const uint32_t seq_len = r0 == 0xffffffffu ? 0u : (uint32_t)v.desc[0][r0].slen;
    if (g == 0) info[kUsSeqLen] = seq_len;
    uint32_t c = 0;
    if (g < n_groups) {
        const uint32_t r = first[g], at = n_groups - 1u - rank[r];
        key[at] = hash[g] % table_size;
        val[at] = g;
        c = count[g];
        uint32_t len = v.desc[0][r].slen;
        if (v.paired) {
            len += v.desc[1][r].slen;
            if (len < seq_len) info[kUsShortKey] = 1u;   // key + strLen points behind the string
            if (len > 1023u) info[kUsLongKey] = 1u;       // pair_seq holds 1024 bytes
        }
    }
    const uint32_t m = wave_max(c);
    if (lane_id() == 0 && m) atomicMax(&info[kUsMaxCount], m);
}

// (the slots in key[] are ascending as they stand: a stable sort of the count's digits leaves equal counts in the walk's order)
__global__ __launch_bounds__(256) void k_usort_count_key(const uint32_t *__restrict__ val, const uint32_t *__restrict__ count,
                                                         uint32_t n_groups, uint64_t *__restrict__ key)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < n_groups) key[q] = (u64)(0xffffffffu - count[val[q]]);
}

// The sequence line of output `mate`: the bytes [a, b) of the joined key
__device__ __forceinline__ void usort_line(uint32_t l0, uint32_t l1, int paired, int mate, uint32_t seq_len, uint32_t &a, uint32_t &b)
{
    const uint32_t len = l0 + (paired ? l1 : 0u);
    const uint32_t cut = seq_len < len ? seq_len : len;
    a = mate ? cut : 0u, b = mate ? len : cut;
}

__global__ __launch_bounds__(256) void k_usort_sizes(UsortView v, int mate, const uint32_t *__restrict__ list,
                                                     const uint32_t *__restrict__ first, const uint32_t *__restrict__ count,
                                                     uint32_t n_groups, uint32_t seq_len, uint64_t *__restrict__ size)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_groups) return;
    const uint32_t g = list[q], r = first[g];
    const UniqDesc d = v.desc[mate][r];
    uint32_t a, b;
    usort_line(v.desc[0][r].slen, v.paired ? v.desc[1][r].slen : 0u, v.paired, mate, seq_len, a, b);
    size[q] = (u64)d.nlen + 1u + uniq_digits(count[g]) + 1u + (b - a) + 3u + d.qlen + 1u;   // "%s\t%ld\n%s\n+\n%s\n"
}

__global__ __launch_bounds__(kTxtThreads) void k_usort_write(UsortView v, int mate, const uint32_t *__restrict__ list,
                                                             const uint32_t *__restrict__ first, const uint32_t *__restrict__ count,
                                                             const uint64_t *__restrict__ off, uint32_t n_groups, uint32_t seq_len,
                                                             uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    const uint8_t *const text = v.text[mate];
    for (uint32_t k0 = wave * kWave; k0 < n_groups; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, dst = 0, p0 = 0, p1 = 0;   // p0, p1: where the line's spans start in text[0] and text[1]
        uint32_t nlen = 0, qlen = 0, qrel = 0, nd = 0, n0 = 0, n1 = 0;
        if (k < n_groups) {
            const uint32_t g = list[k], r = first[g];
            const UniqDesc d0 = v.desc[0][r];
            const UniqDesc d = mate ? v.desc[1][r] : d0;
            const uint32_t l0 = d0.slen, l1 = mate ? d.slen : v.paired ? (uint32_t)v.desc[1][r].slen : 0u;
            uint32_t a, b;
            usort_line(l0, l1, v.paired, mate, seq_len, a, b);
            if (a < l0) p0 = d0.off + d0.nlen + 1u + a, n0 = (b < l0 ? b : l0) - a;
            if (b > l0) {   // (pairs only)
                const UniqDesc d1 = v.desc[1][r];
                const uint32_t from = a > l0 ? a - l0 : 0u;
                p1 = d1.off + d1.nlen + 1u + from, n1 = b - l0 - from;
            }
            src = d.off, dst = off[k];
            nlen = d.nlen, qlen = d.qlen, qrel = d.qrel;
            uint32_t c = count[g];
            nd = uniq_digits(c);
            uint8_t *o = out + dst + nlen;   // the fixed bytes and the count, by the record's own lane
            o[0] = '\t';
            for (uint32_t i = nd; i > 0; --i) o[i] = (uint8_t)('0' + c % 10u), c /= 10u;
            o[nd + 1u] = '\n';
            o += nd + 2u + n0 + n1;
            o[0] = '\n', o[1] = '+', o[2] = '\n';
            o[3u + qlen] = '\n';
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n_groups) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave), p0j = __shfl(p0, j, kWave), p1j = __shfl(p1, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), mj = __shfl(qlen, j, kWave), rj = __shfl(qrel, j, kWave);
            const uint32_t ndj = __shfl(nd, j, kWave), n0j = __shfl(n0, j, kWave), n1j = __shfl(n1, j, kWave);
            if (k0 + (uint32_t)j >= n_groups) continue;
            uint8_t *o = out + dj;
            copy_span(text + sj, o, nj, sub);
            o += nj + 2u + ndj;
            copy_span(v.text[0] + p0j, o, n0j, sub);
            if (n1j) copy_span(v.text[1] + p1j, o + n0j, n1j, sub);
            copy_span(text + sj + rj, o + n0j + n1j + 3u, mj, sub);
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned blocks256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }

static UsortView make_view(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired)
{
    UsortView v;
    v.text[0] = t0, v.text[1] = paired ? t1 : t0, v.desc[0] = (const UniqDesc *)d0, v.desc[1] = (const UniqDesc *)(paired ? d1 : d0);
    v.paired = paired;
    return v;
}

hipError_t launch_usort_seqlen(const void *d0, uint32_t n, uint32_t *d_info, hipStream_t st)
{
    hipLaunchKernelGGL(k_usort_seqlen, dim3(blocks256(n)), dim3(256), 0, st, (const UniqDesc *)d0, n, d_info);
    return hipGetLastError();
}

hipError_t launch_usort_djb64(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint32_t *d_first,
                              uint32_t n_groups, uint64_t *d_hash, hipStream_t st)
{
    if (n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(k_usort_djb64, dim3((n_groups + 15u) / 16u), dim3(256), 0, st, make_view(t0, d0, t1, d1, paired), d_first, n_groups,
                       d_hash);
    return hipGetLastError();
}

hipError_t launch_usort_bucket(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint32_t *d_first,
                               const uint32_t *d_rank, const uint32_t *d_count, const uint64_t *d_hash, uint32_t n_groups,
                               uint64_t table_size, uint64_t *d_key, uint32_t *d_val, uint32_t *d_info, hipStream_t st)
{
    hipLaunchKernelGGL(k_usort_bucket, dim3(blocks256(n_groups)), dim3(256), 0, st, make_view(t0, d0, t1, d1, paired), d_first, d_rank,
                       d_count, d_hash, n_groups, (u64)(table_size ? table_size : 1u), d_key, d_val, d_info);
    return hipGetLastError();
}

hipError_t launch_usort_count_key(const uint32_t *d_val, const uint32_t *d_count, uint32_t n_groups, uint64_t *d_key, hipStream_t st)
{
    hipLaunchKernelGGL(k_usort_count_key, dim3(blocks256(n_groups)), dim3(256), 0, st, d_val, d_count, n_groups, d_key);
    return hipGetLastError();
}

hipError_t launch_usort_sizes(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, int mate,
                              const uint32_t *d_list, const uint32_t *d_first, const uint32_t *d_count, uint32_t n_groups, uint32_t seq_len,
                              uint64_t *d_size, hipStream_t st)
{
    hipLaunchKernelGGL(k_usort_sizes, dim3(blocks256(n_groups)), dim3(256), 0, st, make_view(t0, d0, t1, d1, paired), mate, d_list, d_first,
                       d_count, n_groups, seq_len, d_size);
    return hipGetLastError();
}

hipError_t launch_usort_write(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, int mate,
                              const uint32_t *d_list, const uint32_t *d_first, const uint32_t *d_count, const uint64_t *d_off,
                              uint32_t n_groups, uint32_t seq_len, uint8_t *d_out, int n_cu, hipStream_t st)
{
    if (n_groups == 0) return hipSuccess;
    const uint64_t want = ((uint64_t)n_groups + kTxtThreads - 1) / kTxtThreads, cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_usort_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, make_view(t0, d0, t1, d1, paired),
                       mate, d_list, d_first, d_count, d_off, n_groups, seq_len, d_out);
    return hipGetLastError();
}

}  // namespace hpn
