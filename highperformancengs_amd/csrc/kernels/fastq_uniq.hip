// fastq_uniq.hip -- gfx950 kernels of hpn_fastq_uniq_* (gzfastq_uniq.c on the device).
//
// The reference reads a record with four gzgets (readNextNode, gzfastq_uniq.c:170-192), keys a chained hash table by
// the sequence (pairs: by both sequences joined), counts each key and keeps the EARLIEST record with the greatest
// quality sum as its representative (:258-272), then walks the table (dict.c) and, single-end, a qsort of the keys.
// Here the whole stream stays in a device store, every record gets a 32-byte descriptor, and the table walk is
// reproduced from its closed form (docs/kernels/fastq_uniq.md) with three stable radix sorts (radix_sort.hpp):
//
//   k_uniq_keys      over a chunk's line index (k_text_lines): validity, then 16 lanes per record fold the sequence
//                    into two polynomial hashes (djb2's 33 modulo 2^32; an odd 64-bit base modulo 2^64, the grouping
//                    hash), both WITHOUT their seed so that a pair's hash follows from its mates', and sum the
//                    quality bytes, 16 per load.
//   k_uniq_names     pairs: the reference's strncmp of the two names; the first failing ordinal by atomicMin.
//   k_uniq_pair      per record (pair): seeded hashes of the key, quality sum, greatest key length.
//   k_uniq_flags     over the order sorted by grouping hash: a record opens a group iff its hash OR ITS BYTES differ
//                    from its predecessor's; equal hashes over different bytes are counted (the host then orders such
//                    runs by their bytes: exactness never rests on the hash).
//   k_uniq_reduce    count, first ordinal, representative (atomicMax of {sumQ, ~ordinal}) per group.
//   k_uniq_reps      unpacks the representative; tells whether one lies behind the last first occurrence (dict.c's
//                    extra doubling, see hpn_uniq.hip).
//   k_uniq_mark / k_uniq_table_key / k_uniq_seq_word / k_uniq_sizes   the sort keys and the output sizes.
//   k_uniq_write     16 lanes per output record: name, '\t', decimal count, sequence, "\n+\n", quality (copy_span).
//
// Bound: HBM everywhere.  keys reads the chunk once (the name lines are skipped) and writes 32 B per record; flags
// reads two sequences per record through the sorted order (scattered 64-byte lines); write reads and writes each
// kept record once.
#include "radix_sort.hpp"
#include "text_common.hpp"
#include "uniq_desc.hpp"

namespace hpn {

struct UniqView {
    const uint8_t *text[2];
    const UniqDesc *desc[2];
    int paired;
};

constexpr u64 kUniqBase = 0x9E3779B97F4A7C15ull;   // odd

__device__ __forceinline__ uint32_t pow33(uint32_t e)   // e < 4096
{
    uint32_t r = 1u, b = 33u;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (e & (1u << k)) r *= b;
        b *= b;
    }
    return r;
}
__device__ __forceinline__ u64 powB(uint32_t e)   // e < 4096
{
    u64 r = 1u, b = kUniqBase;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (e & (1u << k)) r *= b;
        b *= b;
    }
    return r;
}

// Launched with an upper bound of workgroups (the line count lives on the device).  st: the state block k_text_lines
// left; desc: where this chunk's first descriptor goes; origin: the store offset of slot[begin].  kShortQual: a quality line two
// or more bytes shorter than its sequence is irregular (gzfastq_uniq.c sums bytes outside its buffer; gzfastq_uniqQ.c prints
// nothing of its sum, so hpn_fastq_uniqq_add takes such lines: sumq is then the sum over the bytes there are).
template <bool kShortQual>
__global__ __launch_bounds__(kTxtThreads) void k_uniq_keys(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl,
                                                           uint32_t begin, uint32_t end, int last, u64 origin,
                                                           UniqDesc *__restrict__ desc, uint32_t *__restrict__ st)
{
    const int tid = threadIdx.x;
    const uint32_t n_lines = st[kTsLines];
    const uint32_t unterminated = st[kTsUnterminated];
    const uint32_t n = n_lines >> 2;
    if (blockIdx.x == 0 && tid == 0) {
        uint32_t f = 0;
        st[kTsRecs] = n;
        uint32_t consumed = n ? nl[4u * n - 1u] + 1u : begin;
        if (consumed > end) consumed = end;  // the virtual newline
        const uint32_t left = end - consumed;
        if (last && left) {
            // one line without its '\n' behind the last record: gzeof is true after the first gzgets, there is no record
            if ((n_lines & 3u) == 1u && unterminated) consumed = end;
            else f |= HPN_TEXT_PARTIAL;
        }
        if (!last && left > 4096u) f |= HPN_TEXT_LONG_LINE;   // (four lines of at most 1023 bytes are 4092)
        st[kTsConsumed] = consumed;
        if (f) atomicOr(&st[kTsFlags], f);
    }
    const uint32_t r = blockIdx.x * kTxtThreads + (uint32_t)tid;
    if ((u64)blockIdx.x * kTxtThreads >= n) return;
    const bool have = r < n;
    uint32_t p0 = 0, l1 = 0, ss = 0, ls = 0, qs = 0, lq = 0;
    if (have) {
        u32 e;
        __builtin_memcpy(&e, nl + 4u * r, 16);
        const uint32_t prev = r ? nl[4u * r - 1u] : begin - 1u;
        const bool open_end = unterminated && r == n - 1u && 4u * n == n_lines;
        p0 = prev + 1u, l1 = e[0] - prev - 1u;
        ss = e[0] + 1u, ls = e[1] - e[0] - 1u;
        qs = e[2] + 1u, lq = e[3] - e[2] - 1u - (open_end ? 1u : 0u);   // a last line without '\n' loses a real byte
        uint32_t f = 0;
        if (e[0] - prev > 1023u || e[1] - e[0] > 1023u || e[2] - e[1] > 1023u || e[3] - e[2] > 1023u) f |= HPN_TEXT_LONG_LINE;  // gzgets would split it
        else if (kShortQual && lq + 1u < ls) f |= HPN_TEXT_SHORT_QUAL;   // the reference would sum bytes outside its buffer
        if (f) {
            atomicOr(&st[kTsFlags], f);
            ls = lq = 0;   // (the chunk is refused anyway: keep the loads inside it)
        }
    }
    const uint32_t lm = lq < ls ? lq : ls;
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    const uint32_t wave_r0 = blockIdx.x * kTxtThreads + (uint32_t)wave_id() * kWave;
    u64 my_h = 0;
    uint32_t my_d = 0, my_q = 0;
    for (int it = 0; it < kWave / 4; ++it) {  // four records per wave-instruction, 16 lanes each
        if (wave_r0 + 4u * (uint32_t)it >= n) break;
        const int j = 4 * it + grp;
        const uint32_t sj = __shfl(ss, j, kWave), lj = __shfl(ls, j, kWave), qj = __shfl(qs, j, kWave), mj = __shfl(lm, j, kWave);
        u64 h = 0;
        uint32_t d = 0, q = 0;
        for (uint32_t o = 16u * (uint32_t)sub; o < lj; o += 256u) {
            u32 w;
            __builtin_memcpy(&w, slot + sj + o, 16);   // (up to 15 bytes beyond the sequence: inside the record)
            const uint32_t cnt = lj - o < 16u ? lj - o : 16u;
            u64 hw = 0;
            uint32_t dw = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 255u;
                if ((uint32_t)i < cnt) hw = hw * kUniqBase + c, dw = dw * 33u + c;
            }
            h += hw * powB(lj - o - cnt);
            d += dw * pow33(lj - o - cnt);
        }
        for (uint32_t o = 16u * (uint32_t)sub; o < mj; o += 256u) {
            u32 w;
            __builtin_memcpy(&w, slot + qj + o, 16);   // (up to 15 bytes beyond the line: the next record, or the store's slack)
            const uint32_t cnt = mj - o < 16u ? mj - o : 16u;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((uint32_t)i < cnt) q += (w[i >> 2] >> (8 * (i & 3))) & 255u;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            h += __shfl_xor(h, o, 16);
            d += __shfl_xor(d, o, 16);
            q += __shfl_xor(q, o, 16);
        }
        // hand the sums to the record's own lane
        const u64 hh = __shfl(h, (lane & 3) * 16, kWave);
        const uint32_t dd = __shfl(d, (lane & 3) * 16, kWave), qq = __shfl(q, (lane & 3) * 16, kWave);
        if ((lane >> 2) == it) my_h = hh, my_d = dd, my_q = qq;
    }
    if (have) {
        UniqDesc x;
        x.off = origin + (p0 - begin);
        x.h0 = my_h, x.d0 = my_d, x.sumq = my_q;
        x.nlen = (uint16_t)l1, x.slen = (uint16_t)ls, x.qlen = (uint16_t)lq, x.qrel = (uint16_t)(qs - p0);
        desc[r] = x;
    }
}

// strncmp(name1, name2, strchr(name1, ' ') - name1) != 0 (gzfastq_uniq.c:207-208): the bytes in front of name 1's first
// space must open name 2; without a space the count is huge and the names must be equal as wholes.
__global__ __launch_bounds__(256) void k_uniq_names(UniqView v, uint32_t n, uint32_t *__restrict__ first_bad)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const UniqDesc a = v.desc[0][i], b = v.desc[1][i];
    const uint8_t *pa = v.text[0] + a.off, *pb = v.text[1] + b.off;
    uint32_t k = 0;
    while (k < a.nlen && pa[k] != ' ') ++k;
    bool bad = k == a.nlen ? a.nlen != b.nlen : b.nlen < k;
    for (uint32_t t = 0; !bad && t < k; ++t) bad = pa[t] != pb[t];
    if (bad) atomicMin(first_bad, i);
}

// info[0]: greatest key length
__global__ __launch_bounds__(256) void k_uniq_pair(UniqView v, uint32_t n, u64 hash_mask, uint64_t *__restrict__ hash,
                                                   uint32_t *__restrict__ order, uint32_t *__restrict__ djb,
                                                   uint32_t *__restrict__ sumq, uint32_t *__restrict__ info)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t L = 0;
    if (i < n) {
        const UniqDesc a = v.desc[0][i];
        L = a.slen;
        u64 h = powB(L) + a.h0;
        uint32_t d = 5381u * pow33(L) + a.d0, q = a.sumq;
        if (v.paired) {
            const UniqDesc b = v.desc[1][i];
            h = h * powB(b.slen) + b.h0;
            d = d * pow33(b.slen) + b.d0;
            q += b.sumq;
            L += b.slen;
        }
        hash[i] = h & hash_mask, order[i] = i, djb[i] = d, sumq[i] = q;
    }
    const uint32_t m = wave_max(L);
    if (lane_id() == 0 && m) atomicMax(&info[0], m);
}

__device__ __forceinline__ bool span_equal(const uint8_t *a, const uint8_t *b, uint32_t len)
{
    uint32_t o = 0;
    for (; o + 16u <= len; o += 16u) {
        u32 x, y;
        __builtin_memcpy(&x, a + o, 16);
        __builtin_memcpy(&y, b + o, 16);
        if (x[0] != y[0] || x[1] != y[1] || x[2] != y[2] || x[3] != y[3]) return false;
    }
    for (; o < len; ++o)
        if (a[o] != b[o]) return false;
    return true;
}

__device__ __forceinline__ bool key_equal(const UniqView &v, uint32_t ra, uint32_t rb)
{
    const UniqDesc a0 = v.desc[0][ra], b0 = v.desc[0][rb];
    const uint8_t *pa0 = v.text[0] + a0.off + a0.nlen + 1u, *pb0 = v.text[0] + b0.off + b0.nlen + 1u;
    if (!v.paired) return a0.slen == b0.slen && span_equal(pa0, pb0, a0.slen);
    const UniqDesc a1 = v.desc[1][ra], b1 = v.desc[1][rb];
    const uint8_t *pa1 = v.text[1] + a1.off + a1.nlen + 1u, *pb1 = v.text[1] + b1.off + b1.nlen + 1u;
    if ((uint32_t)a0.slen + a1.slen != (uint32_t)b0.slen + b1.slen) return false;
    if (a0.slen == b0.slen) return span_equal(pa0, pb0, a0.slen) && span_equal(pa1, pb1, a1.slen);
    const uint32_t L = (uint32_t)a0.slen + a1.slen;   // the same bytes cut at another place
    for (uint32_t t = 0; t < L; ++t) {
        const uint8_t x = t < a0.slen ? pa0[t] : pa1[t - a0.slen], y = t < b0.slen ? pb0[t] : pb1[t - b0.slen];
        if (x != y) return false;
    }
    return true;
}

// info[1]: records whose hash equals their predecessor's while their bytes differ
__global__ __launch_bounds__(256) void k_uniq_flags(UniqView v, const uint64_t *__restrict__ hash, const uint32_t *__restrict__ order,
                                                    uint32_t n, uint32_t *__restrict__ flag, uint32_t *__restrict__ info)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    uint32_t clash = 0;
    if (p < n) {
        uint32_t f = 1;
        if (p && hash[p] == hash[p - 1u]) {
            f = key_equal(v, order[p - 1u], order[p]) ? 0u : 1u;
            clash = f;
        }
        flag[p] = f;
    }
    const uint32_t c = wave_sum(clash);
    if (lane_id() == 0 && c) atomicAdd(&info[1], c);
}

// gid: the exclusive scan of flag; a record's group is gid[p] + flag[p] - 1.  info[2]: the last first occurrence.
__global__ __launch_bounds__(256) void k_uniq_reduce(const uint32_t *__restrict__ order, const uint32_t *__restrict__ flag,
                                                     const uint32_t *__restrict__ gid, const uint32_t *__restrict__ sumq, uint32_t n,
                                                     uint32_t *__restrict__ count, u64 *__restrict__ best,
                                                     uint32_t *__restrict__ first, uint32_t *__restrict__ info)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    uint32_t opened = 0;
    if (p < n) {
        const uint32_t g = gid[p] + flag[p] - 1u, r = order[p];
        atomicAdd(&count[g], 1u);
        atomicMax(&best[g], ((u64)sumq[r] << 32) | (0xffffffffu - r));   // the greatest sum, and among those the least ordinal
        if (flag[p]) first[g] = r, opened = r + 1u;   // (the sorts are stable: a group's records are in file order)
    }
    const uint32_t m = wave_max(opened);
    if (lane_id() == 0 && m) atomicMax(&info[2], m - 1u);
}

// info[3]: set when a representative lies behind the last first occurrence
__global__ __launch_bounds__(256) void k_uniq_reps(const u64 *__restrict__ best, uint32_t n_groups, uint32_t *__restrict__ rep,
                                                   uint32_t *__restrict__ info)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t r = 0xffffffffu - (uint32_t)best[g];
    rep[g] = r;
    if (r > info[2]) atomicOr(&info[3], 1u);
}

__global__ __launch_bounds__(256) void k_uniq_mark(const uint32_t *__restrict__ first, uint32_t n_groups, uint32_t *__restrict__ mark)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_groups) mark[first[g]] = 1u;
}

// rank[r]: the number of first occurrences in front of record r.  The key's place in dict.c's walk:
// ascending (djb2 & (S - 1), p, p ? j : -j) with p = (K - e(j)) & 1, e(j) = 0 for j < 4, else floor(log2 j) - 1.
__global__ __launch_bounds__(256) void k_uniq_table_key(const uint32_t *__restrict__ first, const uint32_t *__restrict__ rank,
                                                        const uint32_t *__restrict__ djb, uint32_t n_groups, uint32_t size_mask,
                                                        uint32_t K, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t r = first[g], j = rank[r];
    const uint32_t e = j < 4u ? 0u : (uint32_t)(31 - __builtin_clz(j)) - 1u;
    const uint32_t p = (K - e) & 1u;
    key[g] = ((u64)(djb[r] & size_mask) << 32) | ((u64)p << 31) | (p ? j : 0x7fffffffu - j);
    val[g] = g;
}

__global__ __launch_bounds__(256) void k_uniq_iota(uint32_t n, uint32_t *__restrict__ val)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) val[g] = g;
}

// The bytes [8 w, 8 w + 8) of a group's sequence, first byte in the top bits, zeros behind its end (no sequence
// holds a NUL byte, so a shorter key comes first among equal prefixes: memcmp, then length -- sdscmp).
__global__ __launch_bounds__(256) void k_uniq_seq_word(UniqView v, const uint32_t *__restrict__ first, const uint32_t *__restrict__ val,
                                                       uint32_t n_groups, uint32_t w, uint64_t *__restrict__ key)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_groups) return;
    const UniqDesc d = v.desc[0][first[val[q]]];
    const uint8_t *s = v.text[0] + d.off + d.nlen + 1u;
    u64 k = 0;
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t at = 8u * w + i;
        k = (k << 8) | (at < d.slen ? s[at] : 0u);
    }
    key[q] = k;
}

__global__ __launch_bounds__(256) void k_uniq_sizes(const UniqDesc *__restrict__ desc, const uint32_t *__restrict__ list,
                                                    const uint32_t *__restrict__ rep, const uint32_t *__restrict__ count,
                                                    uint32_t n_groups, uint32_t *__restrict__ size)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_groups) return;
    const uint32_t g = list[q];
    const UniqDesc d = desc[rep[g]];
    size[q] = (uint32_t)d.nlen + 1u + uniq_digits(count[g]) + 1u + d.slen + 3u + d.qlen + 1u;   // "%s\t%u\n%s\n+\n%s\n"
}

__global__ __launch_bounds__(kTxtThreads) void k_uniq_write(const uint8_t *__restrict__ text, const UniqDesc *__restrict__ desc,
                                                            const uint32_t *__restrict__ list, const uint32_t *__restrict__ rep,
                                                            const uint32_t *__restrict__ count, const uint64_t *__restrict__ off,
                                                            uint32_t n_groups, uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n_groups; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, dst = 0;
        uint32_t nlen = 0, slen = 0, qlen = 0, qrel = 0, nd = 0;
        if (k < n_groups) {
            const uint32_t g = list[k];
            const UniqDesc d = desc[rep[g]];
            src = d.off, dst = off[k];
            nlen = d.nlen, slen = d.slen, qlen = d.qlen, qrel = d.qrel;
            uint32_t c = count[g];
            nd = uniq_digits(c);
            uint8_t *o = out + dst + nlen;   // the fixed bytes and the count, by the record's own lane
            o[0] = '\t';
            for (uint32_t i = nd; i > 0; --i) o[i] = (uint8_t)('0' + c % 10u), c /= 10u;
            o[nd + 1u] = '\n';
            o += nd + 2u + slen;
            o[0] = '\n', o[1] = '+', o[2] = '\n';
            o[3u + qlen] = '\n';
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n_groups) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), cj = __shfl(slen, j, kWave), mj = __shfl(qlen, j, kWave);
            const uint32_t rj = __shfl(qrel, j, kWave), ndj = __shfl(nd, j, kWave);
            if (k0 + (uint32_t)j >= n_groups) continue;
            uint8_t *o = out + dj;
            copy_span(text + sj, o, nj, sub);
            copy_span(text + sj + nj + 1u, o + nj + 2u + ndj, cj, sub);
            copy_span(text + sj + rj, o + nj + 2u + ndj + cj + 3u, mj, sub);
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned blocks256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }

hipError_t launch_uniq_keys(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                            void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *)
{
    hipLaunchKernelGGL(k_uniq_keys<true>, dim3(max_records / kTxtThreads + 1u), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, end, last,
                       (u64)origin, (UniqDesc *)d_desc, d_state);
    return hipGetLastError();
}

hipError_t launch_uniqq_keys(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                             void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *)
{
    hipLaunchKernelGGL(k_uniq_keys<false>, dim3(max_records / kTxtThreads + 1u), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, end, last,
                       (u64)origin, (UniqDesc *)d_desc, d_state);
    return hipGetLastError();
}

static UniqView make_view(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired)
{
    UniqView v;
    v.text[0] = t0, v.text[1] = t1, v.desc[0] = (const UniqDesc *)d0, v.desc[1] = (const UniqDesc *)d1, v.paired = paired;
    return v;
}

hipError_t launch_uniq_names(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, uint32_t n, uint32_t *d_first_bad,
                             hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_names, dim3(blocks256(n)), dim3(256), 0, st, make_view(t0, d0, t1, d1, 1), n, d_first_bad);
    return hipGetLastError();
}

hipError_t launch_uniq_pair(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, uint32_t n,
                            uint64_t hash_mask, uint64_t *d_hash, uint32_t *d_order, uint32_t *d_djb, uint32_t *d_sumq, uint32_t *d_info,
                            hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_pair, dim3(blocks256(n)), dim3(256), 0, st, make_view(t0, d0, t1, d1, paired), n, (u64)hash_mask, d_hash,
                       d_order, d_djb, d_sumq, d_info);
    return hipGetLastError();
}

hipError_t launch_uniq_flags(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint64_t *d_hash,
                             const uint32_t *d_order, uint32_t n, uint32_t *d_flag, uint32_t *d_info, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_flags, dim3(blocks256(n)), dim3(256), 0, st, make_view(t0, d0, t1, d1, paired), d_hash, d_order, n, d_flag,
                       d_info);
    return hipGetLastError();
}

hipError_t launch_uniq_reduce(const uint32_t *d_order, const uint32_t *d_flag, const uint32_t *d_gid, const uint32_t *d_sumq, uint32_t n,
                              uint32_t n_groups, uint32_t *d_count, uint64_t *d_best, uint32_t *d_first, uint32_t *d_rep, uint32_t *d_info,
                              hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_count, 0, (size_t)n_groups * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_best, 0, (size_t)n_groups * sizeof(uint64_t), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_uniq_reduce, dim3(blocks256(n)), dim3(256), 0, st, d_order, d_flag, d_gid, d_sumq, n, d_count, (u64 *)d_best,
                       d_first, d_info);
    hipLaunchKernelGGL(k_uniq_reps, dim3(blocks256(n_groups)), dim3(256), 0, st, (const u64 *)d_best, n_groups, d_rep, d_info);
    return hipGetLastError();
}

hipError_t launch_uniq_mark(const uint32_t *d_first, uint32_t n_groups, uint32_t *d_mark, uint32_t n, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_mark, 0, (size_t)n * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_uniq_mark, dim3(blocks256(n_groups)), dim3(256), 0, st, d_first, n_groups, d_mark);
    return hipGetLastError();
}

hipError_t launch_uniq_table_key(const uint32_t *d_first, const uint32_t *d_rank, const uint32_t *d_djb, uint32_t n_groups,
                                 uint32_t size_mask, uint32_t K, uint64_t *d_key, uint32_t *d_val, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_table_key, dim3(blocks256(n_groups)), dim3(256), 0, st, d_first, d_rank, d_djb, n_groups, size_mask, K, d_key,
                       d_val);
    return hipGetLastError();
}

hipError_t launch_uniq_iota(uint32_t n, uint32_t *d_val, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_iota, dim3(blocks256(n)), dim3(256), 0, st, n, d_val);
    return hipGetLastError();
}

hipError_t launch_uniq_seq_word(const uint8_t *t0, const void *d0, const uint32_t *d_first, const uint32_t *d_val, uint32_t n_groups,
                                uint32_t w, uint64_t *d_key, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_seq_word, dim3(blocks256(n_groups)), dim3(256), 0, st, make_view(t0, d0, nullptr, nullptr, 0), d_first,
                       d_val, n_groups, w, d_key);
    return hipGetLastError();
}

hipError_t launch_uniq_sizes(const void *d_desc, const uint32_t *d_list, const uint32_t *d_rep, const uint32_t *d_count, uint32_t n_groups,
                             uint32_t *d_size, hipStream_t st)
{
    hipLaunchKernelGGL(k_uniq_sizes, dim3(blocks256(n_groups)), dim3(256), 0, st, (const UniqDesc *)d_desc, d_list, d_rep, d_count,
                       n_groups, d_size);
    return hipGetLastError();
}

hipError_t launch_uniq_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_list, const uint32_t *d_rep,
                             const uint32_t *d_count, const uint64_t *d_off, uint32_t n_groups, uint8_t *d_out, int n_cu, hipStream_t st)
{
    if (n_groups == 0) return hipSuccess;
    uint64_t want = ((uint64_t)n_groups + kTxtThreads - 1) / kTxtThreads;
    const uint64_t cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_uniq_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, d_text, (const UniqDesc *)d_desc,
                       d_list, d_rep, d_count, d_off, n_groups, d_out);
    return hipGetLastError();
}

hipError_t uniq_scan32(const uint32_t *d_in, uint32_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st)
{
    return launch_excl_scan<uint32_t, uint32_t>(d_in, d_out, n, d_status, d_ticket, d_err, st);
}
hipError_t uniq_scan64(const uint32_t *d_in, uint64_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st)
{
    return launch_excl_scan<uint32_t, uint64_t>(d_in, d_out, n, d_status, d_ticket, d_err, st);
}
// 64-bit items (hpn_fastq_uniqq_*: a group's bytes -- one group of quality lines can pass 4 GiB)
hipError_t uniq_scan64w(const uint64_t *d_in, uint64_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st)
{
    return launch_excl_scan<uint64_t, uint64_t>(d_in, d_out, n, d_status, d_ticket, d_err, st);
}
uint64_t uniq_scan_tiles(uint64_t n) { return scan_tiles(n); }
uint64_t uniq_sort_hist_words(uint32_t n) { return sort_hist_words(n); }
hipError_t uniq_sort_pairs(uint64_t *d_keys, uint32_t *d_vals, uint32_t n, int begin_bit, int end_bit, uint64_t *d_keys_tmp,
                           uint32_t *d_vals_tmp, uint32_t *d_hist, uint32_t *d_offs, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err,
                           hipStream_t st)
{
    const SortSpace ws{d_keys_tmp, d_vals_tmp, d_hist, d_offs, d_status, d_ticket, d_err};
    return radix_sort_pairs(d_keys, d_vals, n, begin_bit, end_bit, ws, st);
}

// radix_sort_pairs over the digits of `digits` only (bit d: the key bits [8 d, 8 d + 8) take part), lowest first: stable, in
// place, one copy back when the number of passes is odd.
hipError_t uniq_sort_pairs_digits(uint64_t *d_keys, uint32_t *d_vals, uint32_t n, uint32_t digits, uint64_t *d_keys_tmp, uint32_t *d_vals_tmp,
                             uint32_t *d_hist, uint32_t *d_offs, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t s)
{
    if (n < 2 || !(digits & 255u)) return hipSuccess;
    const uint32_t tiles = sort_tiles(n);
    const unsigned grid = (tiles + kSortThreads / kWave - 1) / (kSortThreads / kWave);
    const size_t hw = (size_t)256 * tiles;
    uint64_t *ka = d_keys, *kb = d_keys_tmp;
    uint32_t *va = d_vals, *vb = d_vals_tmp;
    for (int d = 0; d < 8; ++d) {
        if (!((digits >> d) & 1u)) continue;
        hipLaunchKernelGGL(k_radix_hist, dim3(grid), dim3(kSortThreads), 0, s, ka, n, 8 * d, 255u, tiles, d_hist);
        hipError_t e = launch_excl_scan<uint32_t, uint32_t>(d_hist, d_offs, hw, d_status, d_ticket, d_err, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_radix_scatter, dim3(grid), dim3(kSortThreads), 0, s, ka, va, n, 8 * d, 255u, tiles, d_offs, kb, vb);
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
