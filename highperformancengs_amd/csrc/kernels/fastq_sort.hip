// fastq_sort.hip -- gfx950 kernels of hpn_fastq_sort_* (gzfastq_sort.c on the device).
//
// The reference reads every record into memory (readNextNode: four gzgets, the last byte of name, sequence and quality
// dropped), qsorts the array by the KEY LINE -- the name line or the sequence line -- first by strlen, then by strcmp, and
// prints "name\nseq\n+\nquality\n".  glibc's qsort is a merge sort there: equal keys keep their input order.  Here the
// stream lies in the device store (hpn_store.hpp) with a 16-byte descriptor per record, and the order
// (length, bytes, input ordinal) is built most significant bytes first, by stable radix sorts (radix_sort.hpp, instantiated
// in fastq_uniq.hip) over fewer and fewer records (docs/kernels/fastq_sort.md):
//
//   k_sort_frame   over a chunk's line index (k_text_lines): validity, one descriptor per record.
//   k_sort_key0    round 0, all N records: key = length << 48 | the first 6 bytes big-endian (zeros behind the end: no line
//                  holds a NUL byte), payload = ordinal.  One 8-byte load per record through its descriptor.
//   k_sort_bits    OR and AND of the keys: the radix passes run only over digits in which two keys differ.
//   k_sort_place0  the sorted ordinals become the order; every record's key pointer and length are gathered ONCE into
//                  arrays that follow the order, so later rounds reach the text through one dependent load.
//   k_sort_heads / k_sort_equal / k_sort_keep / k_sort_compact
//                  a run = the records that agree in length and in all bytes sorted so far.  A record that opens no run is
//                  compared with its predecessor over the REMAINING bytes, 16 per load, up to the first difference; a run
//                  in which no such pair differs is settled (duplicates, and every run whose bytes are used up).  The
//                  records of the other runs are compacted, their positions in the order with them.
//   k_sort_word    round k >= 1, the tied records only: key = the next 8 bytes, payload = index.  Sorted by that word and
//                  then by run number (both stable), the i-th element belongs at the i-th tied position:
//   k_sort_runkey / k_sort_place   the second sort's key, and the write-back.
//   k_sort_sizes + scan, k_sort_write   the output text, 16 lanes per record (copy_span).
//
// A third key mode beside name and sequence (hpn_kseq_*: std::map<std::string>'s order, strcmp): the sequence's bytes alone,
// zero-padded, without the length in front.  Round 0's key then carries no length (`bytes_only`), and a run is settled only
// when its neighbours agree in length AS WELL AS in bytes: a key that is a proper prefix of its neighbour stays, and the zero
// word it gets in the next round puts it in front.
//
// Bound: HBM.  Round 0 and the output touch every record; on reads, round 1 touches nearly all of them once more (4^6
// prefixes) and round 2 a few thousand.  The scattered loads (key0: descriptor then text; word, equal: text) are issued for
// several records per lane before the first is used.
#include "sort_desc.hpp"
#include "text_common.hpp"

namespace hpn {

constexpr uint32_t kSortItems = 4;   // records per lane where the loads are scattered

// Launched with an upper bound of workgroups (the line count lives on the device).  st: the state block k_text_lines left;
// desc: where this chunk's first descriptor goes; origin: the store offset of slot[begin].
__global__ __launch_bounds__(kTxtThreads) void k_sort_frame(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl,
                                                            uint32_t begin, uint32_t end, int last, u64 origin,
                                                            SortDesc *__restrict__ desc, uint32_t *__restrict__ st)
{
    const uint32_t n_lines = st[kTsLines];
    const uint32_t unterminated = st[kTsUnterminated];
    const uint32_t n = n_lines >> 2;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
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
    const uint32_t r = blockIdx.x * kTxtThreads + threadIdx.x;
    if (r >= n) return;
    u32 e;
    __builtin_memcpy(&e, nl + 4u * r, 16);
    const uint32_t prev = r ? nl[4u * r - 1u] : begin - 1u;
    const bool open_end = unterminated && r == n - 1u && 4u * n == n_lines;
    if (e[0] - prev > 1023u || e[1] - e[0] > 1023u || e[2] - e[1] > 1023u || e[3] - e[2] > 1023u) {
        atomicOr(&st[kTsFlags], HPN_TEXT_LONG_LINE);   // gzgets would split it
        return;
    }
    const uint32_t p0 = prev + 1u;
    SortDesc x;
    x.off = origin + (p0 - begin);
    x.nlen = (uint16_t)(e[0] - prev - 1u), x.slen = (uint16_t)(e[1] - e[0] - 1u);
    x.qlen = (uint16_t)(e[3] - e[2] - 1u - (open_end ? 1u : 0u));   // a last line without '\n' loses a real byte
    x.qrel = (uint16_t)(e[2] + 1u - p0);
    desc[r] = x;
}

__global__ __launch_bounds__(256) void k_sort_key0(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc, int by_name,
                                                   int bytes_only, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * kSortItems;
    SortDesc d[kSortItems];
    u64 w[kSortItems];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (i0 + k < n) d[k] = desc[i0 + k];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (i0 + k < n) __builtin_memcpy(&w[k], text + d[k].off + (by_name ? 0u : (uint32_t)d[k].nlen + 1u), 8);
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (i0 + k < n) {
            const uint32_t len = by_name ? d[k].nlen : d[k].slen, avail = len < 6u ? len : 6u;
            u64 b = __builtin_bswap64(w[k]);
            b = avail ? (b >> (8u * (8u - avail))) << (8u * (8u - avail)) : 0ull;
            key[i0 + k] = ((u64)(bytes_only ? 0u : len) << 48) | (b >> 16);
            val[i0 + k] = i0 + k;
        }
}

// bits[0] |= every key, bits[1] &= every key (the launcher sets them to 0 and ~0)
__global__ __launch_bounds__(256) void k_sort_bits(const uint64_t *__restrict__ key, uint32_t n, u64 *__restrict__ bits)
{
    u64 o = 0, a = ~0ull;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const u64 k = key[i];
        o |= k, a &= k;
    }
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
        o |= __shfl_xor(o, s, kWave);
        a &= __shfl_xor(a, s, kWave);
    }
    if (lane_id() == 0) {
        atomicOr(&bits[0], o);
        atomicAnd(&bits[1], a);
    }
}

// the tied records' arrays, in the order's direction: position in the order, ordinal, key pointer (store offset), key length, run
struct SortTied {
    uint32_t *pos, *ord, *len, *run;
    u64 *kp;
};

__global__ __launch_bounds__(256) void k_sort_place0(const SortDesc *__restrict__ desc, int by_name, const uint32_t *__restrict__ val,
                                                     uint32_t n, uint32_t *__restrict__ order, SortTied t)
{
    const uint32_t j0 = (blockIdx.x * 256u + threadIdx.x) * kSortItems;
    uint32_t r[kSortItems];
    SortDesc d[kSortItems];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (j0 + k < n) r[k] = val[j0 + k];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (j0 + k < n) d[k] = desc[r[k]];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (j0 + k < n) {
            const uint32_t j = j0 + k;
            order[j] = r[k];
            t.pos[j] = j, t.ord[j] = r[k], t.run[j] = 0u;
            t.kp[j] = d[k].off + (by_name ? 0u : (uint32_t)d[k].nlen + 1u);
            t.len[j] = by_name ? d[k].nlen : d[k].slen;
        }
}

// head[j]: element j opens a run -- its run of the round before, or the word just sorted by, differs from its predecessor's
__global__ __launch_bounds__(256) void k_sort_heads(const uint64_t *__restrict__ word, const uint32_t *__restrict__ run, uint32_t m,
                                                    uint32_t *__restrict__ head)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    head[j] = (j == 0u || run[j] != run[j - 1u] || word[j] != word[j - 1u]) ? 1u : 0u;
}

// do the `len` bytes at a and b differ?  16 per load, up to the first difference (the last load may reach up to 15 bytes
// behind the spans: the next line, or the store's slack)
__device__ __forceinline__ bool span_differs(const uint8_t *a, const uint8_t *b, uint32_t len)
{
    for (uint32_t o = 0; o < len; o += 16u) {
        u32 x, y;
        __builtin_memcpy(&x, a + o, 16);
        __builtin_memcpy(&y, b + o, 16);
        const uint32_t rem = len - o;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            uint32_t df = x[q] ^ y[q];
            if (rem < 4u * q + 4u) df = rem > 4u * q ? df & (0xffffffffu >> (8u * (4u * q + 4u - rem))) : 0u;   // (little-endian: the first byte is the lowest)
            if (df) return true;
        }
    }
    return false;
}

// gid: the exclusive scan of head; element j's run is gid[j] + head[j] - 1.  c: the key bytes sorted so far.  stay[run] is set
// when two neighbours of the run differ behind byte c (a run shorter than that, or of equal keys, is settled).
__global__ __launch_bounds__(256) void k_sort_equal(const uint8_t *__restrict__ text, const u64 *__restrict__ kp,
                                                    const uint32_t *__restrict__ len, const uint32_t *__restrict__ head,
                                                    const uint32_t *__restrict__ gid, uint32_t c, uint32_t m, int bytes_only,
                                                    uint32_t *__restrict__ stay)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m || j == 0u || head[j]) return;
    const uint32_t L = len[j];
    if (bytes_only && len[j - 1u] != L) {   // one is a proper prefix of the other so far: the padding decides
        stay[gid[j] - 1u] = 1u;
        return;
    }
    if (L <= c) return;
    if (span_differs(text + kp[j] + c, text + kp[j - 1u] + c, L - c)) stay[gid[j] - 1u] = 1u;
}

__global__ __launch_bounds__(256) void k_sort_keep(const uint32_t *__restrict__ head, const uint32_t *__restrict__ gid,
                                                   const uint32_t *__restrict__ stay, uint32_t m, uint32_t *__restrict__ keep)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < m) keep[j] = stay[gid[j] + head[j] - 1u];
}

// at: the exclusive scan of keep
__global__ __launch_bounds__(256) void k_sort_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ at,
                                                      const uint32_t *__restrict__ head, const uint32_t *__restrict__ gid, SortTied a,
                                                      uint32_t m, SortTied b)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m || !keep[j]) return;
    const uint32_t d = at[j];
    b.pos[d] = a.pos[j], b.ord[d] = a.ord[j], b.len[d] = a.len[j], b.kp[d] = a.kp[j];
    b.run[d] = gid[j] + head[j] - 1u;
}

__global__ __launch_bounds__(256) void k_sort_word(const uint8_t *__restrict__ text, const u64 *__restrict__ kp,
                                                   const uint32_t *__restrict__ len, uint32_t c, uint32_t m, uint64_t *__restrict__ key,
                                                   uint32_t *__restrict__ val)
{
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * kSortItems;
    u64 p[kSortItems], w[kSortItems];
    uint32_t L[kSortItems];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (i0 + k < m) p[k] = kp[i0 + k], L[k] = len[i0 + k];
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (i0 + k < m) __builtin_memcpy(&w[k], text + p[k] + c, 8);
#pragma unroll
    for (uint32_t k = 0; k < kSortItems; ++k)
        if (i0 + k < m) {
            const uint32_t avail = L[k] > c ? (L[k] - c < 8u ? L[k] - c : 8u) : 0u;
            const u64 b = __builtin_bswap64(w[k]);
            key[i0 + k] = avail >= 8u ? b : avail ? (b >> (8u * (8u - avail))) << (8u * (8u - avail)) : 0ull;
            val[i0 + k] = i0 + k;
        }
}

// the second sort of a round: by the run of the element that the first sort put at i; its payload is i itself
__global__ __launch_bounds__(256) void k_sort_runkey(const uint32_t *__restrict__ run, const uint32_t *__restrict__ val1, uint32_t m,
                                                     uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    key[i] = run[val1[i]];
    val[i] = i;
}

// val2[j] = i: the element the first sort put at i -- a.*[val1[i]], whose word is word1[i] -- belongs at the j-th tied position
__global__ __launch_bounds__(256) void k_sort_place(const uint32_t *__restrict__ val2, const uint32_t *__restrict__ val1,
                                                    const uint64_t *__restrict__ word1, SortTied a, uint32_t m, SortTied b,
                                                    uint64_t *__restrict__ word, uint32_t *__restrict__ order)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = val2[j], s = val1[i];
    const uint32_t r = a.ord[s], p = a.pos[j];
    b.pos[j] = p, b.run[j] = a.run[j];
    b.ord[j] = r, b.len[j] = a.len[s], b.kp[j] = a.kp[s];
    word[j] = word1[i];
    order[p] = r;
}

__global__ __launch_bounds__(256) void k_sort_sizes(const SortDesc *__restrict__ desc, const uint32_t *__restrict__ order, uint32_t n,
                                                    uint32_t *__restrict__ size)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const SortDesc d = desc[order[q]];
    size[q] = (uint32_t)d.nlen + 1u + d.slen + 3u + d.qlen + 1u;   // "%s\n%s\n+\n%s\n"
}

__global__ __launch_bounds__(kTxtThreads) void k_sort_write(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc,
                                                            const uint32_t *__restrict__ order, const uint64_t *__restrict__ off,
                                                            uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, dst = 0;
        uint32_t nlen = 0, slen = 0, qlen = 0, qrel = 0;
        if (k < n) {
            const SortDesc d = desc[order[k]];
            src = d.off, dst = off[k];
            nlen = d.nlen, slen = d.slen, qlen = d.qlen, qrel = d.qrel;
            uint8_t *o = out + dst + nlen;   // the fixed bytes, by the record's own lane
            o[0] = '\n';
            o += 1u + slen;
            o[0] = '\n', o[1] = '+', o[2] = '\n';
            o[3u + qlen] = '\n';
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), cj = __shfl(slen, j, kWave), mj = __shfl(qlen, j, kWave);
            const uint32_t rj = __shfl(qrel, j, kWave);
            if (k0 + (uint32_t)j >= n) continue;
            uint8_t *o = out + dj;
            copy_span(text + sj, o, nj, sub);
            copy_span(text + sj + nj + 1u, o + nj + 1u, cj, sub);
            copy_span(text + sj + rj, o + nj + 1u + cj + 3u, mj, sub);
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned blocks256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }
static inline unsigned blocks_items(uint32_t n) { return blocks256((n + kSortItems - 1u) / kSortItems); }

hipError_t launch_sort_frame(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                             void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *)
{
    hipLaunchKernelGGL(k_sort_frame, dim3(max_records / kTxtThreads + 1u), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, end, last,
                       (u64)origin, (SortDesc *)d_desc, d_state);
    return hipGetLastError();
}

hipError_t launch_sort_key0(const uint8_t *d_text, const void *d_desc, int by_name, int bytes_only, uint32_t n, uint64_t *d_key,
                            uint32_t *d_val, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_key0, dim3(blocks_items(n)), dim3(256), 0, st, d_text, (const SortDesc *)d_desc, by_name, bytes_only, n, d_key,
                       d_val);
    return hipGetLastError();
}

// d_bits: two words, {OR, AND} of the n keys ({0, ~0} without keys)
hipError_t launch_sort_bits(const uint64_t *d_key, uint32_t n, uint64_t *d_bits, int n_cu, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_bits, 0, 8, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_bits + 1, 0xff, 8, st)) != hipSuccess) return e;
    if (!n) return hipSuccess;
    const unsigned want = blocks256(n), cap = (unsigned)n_cu * 8u;
    hipLaunchKernelGGL(k_sort_bits, dim3(want < cap ? want : cap), dim3(256), 0, st, d_key, n, (u64 *)d_bits);
    return hipGetLastError();
}

hipError_t launch_sort_place0(const void *d_desc, int by_name, const uint32_t *d_val, uint32_t n, uint32_t *d_order, const SortTied &t,
                              hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_place0, dim3(blocks_items(n)), dim3(256), 0, st, (const SortDesc *)d_desc, by_name, d_val, n, d_order, t);
    return hipGetLastError();
}

hipError_t launch_sort_heads(const uint64_t *d_word, const uint32_t *d_run, uint32_t m, uint32_t *d_head, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_heads, dim3(blocks256(m)), dim3(256), 0, st, d_word, d_run, m, d_head);
    return hipGetLastError();
}

// d_stay: one word per run (at most m), zeroed here; d_keep[j]: element j's run goes on
hipError_t launch_sort_settle(const uint8_t *d_text, const SortTied &t, const uint32_t *d_head, const uint32_t *d_gid, uint32_t c,
                              uint32_t m, int bytes_only, uint32_t *d_stay, uint32_t *d_keep, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_stay, 0, (size_t)m * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sort_equal, dim3(blocks256(m)), dim3(256), 0, st, d_text, t.kp, t.len, d_head, d_gid, c, m, bytes_only, d_stay);
    hipLaunchKernelGGL(k_sort_keep, dim3(blocks256(m)), dim3(256), 0, st, d_head, d_gid, d_stay, m, d_keep);
    return hipGetLastError();
}

hipError_t launch_sort_compact(const uint32_t *d_keep, const uint32_t *d_at, const uint32_t *d_head, const uint32_t *d_gid,
                               const SortTied &a, uint32_t m, const SortTied &b, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_compact, dim3(blocks256(m)), dim3(256), 0, st, d_keep, d_at, d_head, d_gid, a, m, b);
    return hipGetLastError();
}

hipError_t launch_sort_word(const uint8_t *d_text, const SortTied &t, uint32_t c, uint32_t m, uint64_t *d_key, uint32_t *d_val,
                            hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_word, dim3(blocks_items(m)), dim3(256), 0, st, d_text, t.kp, t.len, c, m, d_key, d_val);
    return hipGetLastError();
}

hipError_t launch_sort_runkey(const uint32_t *d_run, const uint32_t *d_val1, uint32_t m, uint64_t *d_key, uint32_t *d_val, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_runkey, dim3(blocks256(m)), dim3(256), 0, st, d_run, d_val1, m, d_key, d_val);
    return hipGetLastError();
}

hipError_t launch_sort_place(const uint32_t *d_val2, const uint32_t *d_val1, const uint64_t *d_word1, const SortTied &a, uint32_t m,
                             const SortTied &b, uint64_t *d_word, uint32_t *d_order, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_place, dim3(blocks256(m)), dim3(256), 0, st, d_val2, d_val1, d_word1, a, m, b, d_word, d_order);
    return hipGetLastError();
}

hipError_t launch_sort_sizes(const void *d_desc, const uint32_t *d_order, uint32_t n, uint32_t *d_size, hipStream_t st)
{
    hipLaunchKernelGGL(k_sort_sizes, dim3(blocks256(n)), dim3(256), 0, st, (const SortDesc *)d_desc, d_order, n, d_size);
    return hipGetLastError();
}

hipError_t launch_sort_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_order, const uint64_t *d_off, uint32_t n,
                             uint8_t *d_out, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    uint64_t want = ((uint64_t)n + kTxtThreads - 1) / kTxtThreads;
    const uint64_t cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_sort_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc,
                       d_order, d_off, n, d_out);
    return hipGetLastError();
}

}  // namespace hpn
