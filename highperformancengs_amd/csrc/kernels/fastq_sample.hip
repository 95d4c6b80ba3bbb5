// fastq_sample.hip -- gfx950 kernels of hpn_fastq_text_sample (gzfastq_sample.c on the device).
//
// The reference reads a record with four gzgets (readNextNode, gzfastq_sample.c:315-335), decides from the
// name line (filter_reads, :150-153: X31 hash + seed, low 24 bits against the fraction) or from a sorted
// list of drawn ordinals (get_number_from_file, :253-264) whether it is kept, and prints a kept one as
// "name_i\nseq\n+\nquality" or ">name_i\nseq\n" (printNode, :30-37) with i its 1-based ordinal.  On regular
// text both are functions of the newline index k_text_lines makes (fastq_text.hip):
//
//   k_sample_select  one lane per record: the validity checks of k_text_records (long line, partial last
//                    record; a quality line of another length than the sequence is regular here, the lines
//                    are copied whole), the keep decision, the size of the output record; one look-back
//                    chain (scan.hpp) scans {bytes, kept} into off[] and the kept ordinals are compacted
//                    into keep[].  Fraction rule: X31 is a polynomial in 31 modulo 2^32, so the 16 lanes of
//                    a group fold one 16-byte word of the name each (every further 256 bytes another) and
//                    the words are combined with powers of 31 -- a name of up to 256 bytes is one load per
//                    lane.  Pick rule: binary search of the ordinal in the uploaded slice of the list.
//   k_sample_write   one lane per KEPT record (dropped ones are never looked at): '_', the decimal ordinal
//                    and the fixed bytes by the record's lane, the three lines by copy_span, 16 lanes each.
//
// Bound: HBM.  select reads 16 B of index per record and the name line (fraction rule) and writes 8 B (+ 8 B
// per kept record); write reads and writes a kept record once.
#include "text_common.hpp"

namespace hpn {

constexpr uint32_t kSmpTile = kTxtThreads;          // records per workgroup of k_sample_select
constexpr int kSmpCountShift = 34;                  // off[]: output bytes below (a chunk is < 2^31 bytes, a record grows by < 24), kept records above (< 2^27)
constexpr u64 kSmpBytesMask = (1ull << kSmpCountShift) - 1;

struct SampleArgs {
    uint32_t mode, fasta, seed_add, threshold;
    const uint64_t *picks;   // device: the ordinals of the list that can fall into this chunk, sorted
    uint32_t n_picks;
    u64 ordinal0;            // 0-based ordinal of the chunk's first record
};

// 31^e modulo 2^32, e < 1024
__device__ __forceinline__ uint32_t pow31(uint32_t e)
{
    uint32_t r = 1u, b = 31u;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        if (e & (1u << k)) r *= b;
        b *= b;
    }
    return r;
}

// h = h * 31 + c over the first cnt bytes of w, c a SIGNED char as in khash.h:336-341 on the reference's platform
__device__ __forceinline__ uint32_t x31_word(u32 w, uint32_t cnt)
{
    uint32_t h = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t c = (uint32_t)(int32_t)(int8_t)(w[i >> 2] >> (8 * (i & 3)));
        if ((uint32_t)i < cnt) h = h * 31u + c;
    }
    return h;
}

__device__ __forceinline__ uint32_t dec_digits(u64 v)
{
    uint32_t d = 1;
    for (u64 p = 10; d < 20u && v >= p; p *= 10) ++d;
    return d;
}

// The fields of a record from its four line ends: name start / length without '\n', sequence start / length,
// quality start / length WITH its '\n' (the last line of a stream that lacks one stays without).
struct SampleRec {
    uint32_t p0, l1, ss, ls, qs, lq;
};
__device__ __forceinline__ SampleRec sample_rec(u32 e, uint32_t prev, bool open_end)
{
    SampleRec f;
    f.p0 = prev + 1u, f.l1 = e[0] - prev - 1u;
    f.ss = e[0] + 1u, f.ls = e[1] - e[0] - 1u;
    f.qs = e[2] + 1u, f.lq = e[3] - e[2] - (open_end ? 1u : 0u);
    return f;
}

// Launched with an upper bound of tiles (the line count lives on the device), like k_text_records.
__global__ __launch_bounds__(kTxtThreads) void k_sample_select(const uint8_t *__restrict__ slot,
                                                               const uint32_t *__restrict__ nl, uint32_t begin,
                                                               uint32_t end, int last, uint32_t carry_cap, SampleArgs a,
                                                               uint64_t *__restrict__ off, uint64_t *__restrict__ keep,
                                                               u64 *__restrict__ status, uint32_t *__restrict__ st)
{
    __shared__ u64 s_wave[kTxtThreads / kWave];
    __shared__ u64 s_excl;
    __shared__ uint32_t s_tile;
    __shared__ uint32_t s_hash[kTxtThreads];
    const int tid = threadIdx.x;
    const uint32_t n_lines = st[kTsLines];
    const uint32_t unterminated = st[kTsUnterminated];
    const uint32_t n = n_lines >> 2;
    if (blockIdx.x == 0 && tid == 0) {
        uint32_t f = 0;
        st[kTsRecs] = n;
        uint32_t consumed = n ? nl[4u * n - 1u] + 1u : begin;
        if (consumed > end) consumed = end;  // the virtual newline
        st[kTsConsumed] = consumed;
        const uint32_t left = end - consumed;
        if (last && left) f |= HPN_TEXT_PARTIAL;
        if (!last && left > carry_cap) f |= HPN_TEXT_LONG_LINE;
        if (f) atomicOr(&st[kTsFlags], f);
        if (n == 0) {
            off[0] = 0;
            st[kTsTotalLo] = st[kTsTotalHi] = st[kTsKept] = 0;
        }
    }
    if ((u64)blockIdx.x * kSmpTile >= n) return;
    if (tid == 0) s_tile = atomicAdd(&st[kTsTicket2], 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint32_t r = tile * kSmpTile + (uint32_t)tid;
    const bool have = r < n;
    SampleRec f = {0, 0, 0, 0, 0, 0};
    if (have) {
        u32 e;
        __builtin_memcpy(&e, nl + 4u * r, 16);
        const uint32_t prev = r ? nl[4u * r - 1u] : begin - 1u;
        if (e[0] - prev > 1023u || e[1] - e[0] > 1023u || e[2] - e[1] > 1023u || e[3] - e[2] > 1023u)
            atomicOr(&st[kTsFlags], (uint32_t)HPN_TEXT_LONG_LINE);  // gzgets would split it
        f = sample_rec(e, prev, unterminated && r == n - 1u && 4u * n == n_lines);
    }
    const u64 g = a.ordinal0 + r;
    bool kept = false;
    if (a.mode == HPN_SAMPLE_FRACTION) {
        const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
        const uint32_t wave_r0 = tile * kSmpTile + (uint32_t)wave_id() * kWave;
        const uint32_t name_len = f.l1 > 1022u ? 0u : f.l1;  // (a long line is refused anyway: keep the loads inside the chunk)
        for (int it = 0; it < kWave / 4; ++it) {  // four records per wave-instruction, 16 lanes each
            if (wave_r0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const uint32_t pj = __shfl(f.p0, j, kWave), lj = __shfl(name_len, j, kWave);
            uint32_t h = 0;
            for (uint32_t o = 16u * (uint32_t)sub; o < lj; o += 256u) {
                u32 w;
                __builtin_memcpy(&w, slot + pj + o, 16);   // (up to 15 bytes beyond the name: inside the record, or the slot's slack)
                const uint32_t cnt = lj - o < 16u ? lj - o : 16u;
                h += x31_word(w, cnt) * pow31(lj - o - cnt);
            }
            h += __shfl_xor(h, 8, 16);
            h += __shfl_xor(h, 4, 16);
            h += __shfl_xor(h, 2, 16);
            h += __shfl_xor(h, 1, 16);
            if (sub == 0) s_hash[wave_id() * kWave + j] = h;
        }
        __syncthreads();
        kept = have && ((s_hash[tid] + a.seed_add) & 0xffffffu) < a.threshold;
    } else if (have) {
        uint32_t lo = 0, hi = a.n_picks;   // first entry >= g
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.picks[mid] < g) lo = mid + 1u;
            else hi = mid;
        }
        kept = lo < a.n_picks && a.picks[lo] == g;
    }
    u64 mine = 0;
    if (kept) {
        const uint32_t head = f.l1 + 1u + dec_digits(g + 1u) + 1u + f.ls;
        mine = (a.fasta ? 1u + head + 1u : head + 3u + f.lq) | (1ull << kSmpCountShift);
    }
    u64 wtotal;
    const u64 wexcl = wave_excl_scan(mine, wtotal);
    if (lane_id() == kWave - 1) s_wave[wave_id()] = wtotal;
    __syncthreads();
    u64 before = 0, aggregate = 0;
#pragma unroll
    for (int w = 0; w < kTxtThreads / kWave; ++w) {
        if (w < wave_id()) before += s_wave[w];
        aggregate += s_wave[w];
    }
    if (wave_id() == 0) {
        const u64 ex = scan_lookback(status, tile, aggregate, &st[kTsErr]);
        if (lane_id() == 0) s_excl = ex;
    }
    __syncthreads();
    const u64 run = s_excl + before + wexcl;
    if (have) {
        off[r] = run;
        if (kept) keep[run >> kSmpCountShift] = g;
        if (r + 1u == n) {
            const u64 all = run + mine;
            off[n] = all;
            st[kTsTotalLo] = (uint32_t)(all & kSmpBytesMask);
            st[kTsTotalHi] = (uint32_t)((all & kSmpBytesMask) >> 32);
            st[kTsKept] = (uint32_t)(all >> kSmpCountShift);
        }
    }
}

__global__ __launch_bounds__(kTxtThreads) void k_sample_write(const uint8_t *__restrict__ slot,
                                                              const uint32_t *__restrict__ nl, uint32_t begin,
                                                              const uint64_t *__restrict__ off,
                                                              const uint64_t *__restrict__ keep, uint32_t n_kept, uint32_t n,
                                                              uint32_t n_lines, uint32_t unterminated, u64 ordinal0,
                                                              uint32_t fasta, uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n_kept; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        SampleRec f = {0, 0, 0, 0, 0, 0};
        uint64_t d = 0;
        uint32_t nd = 0;
        if (k < n_kept) {
            const u64 g = keep[k];
            const uint32_t r = (uint32_t)(g - ordinal0);
            u32 e;
            __builtin_memcpy(&e, nl + 4u * r, 16);
            f = sample_rec(e, r ? nl[4u * r - 1u] : begin - 1u, unterminated && r == n - 1u && 4u * n == n_lines);
            d = off[r] & kSmpBytesMask;
            // "_%lu\n" and the fixed bytes behind the sequence, by the record's own lane
            u64 v = g + 1u;
            nd = dec_digits(v);
            uint8_t *o = out + d + fasta;
            if (fasta) o[-1] = '>';
            o[f.l1] = '_';
            for (uint32_t i = nd; i > 0; --i) {
                if (v >> 32) {
                    o[f.l1 + i] = (uint8_t)('0' + (uint32_t)(v % 10u));
                    v /= 10u;
                } else {
                    const uint32_t v32 = (uint32_t)v;
                    o[f.l1 + i] = (uint8_t)('0' + v32 % 10u);
                    v = v32 / 10u;
                }
            }
            o[f.l1 + 1u + nd] = '\n';
            const uint32_t t = f.l1 + 2u + nd + f.ls;
            o[t] = '\n';
            if (!fasta) o[t + 1u] = '+', o[t + 2u] = '\n';
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n_kept) break;
            const int j = 4 * it + grp;
            const uint32_t pj = __shfl(f.p0, j, kWave), lj = __shfl(f.l1, j, kWave), sj = __shfl(f.ss, j, kWave);
            const uint32_t cj = __shfl(f.ls, j, kWave), qj = __shfl(f.qs, j, kWave), mj = __shfl(f.lq, j, kWave);
            const uint32_t ndj = __shfl(nd, j, kWave);
            const uint64_t dj = __shfl(d, j, kWave);
            if (k0 + (uint32_t)j >= n_kept) continue;
            uint8_t *o = out + dj + fasta;
            copy_span(slot + pj, o, lj, sub);                                   // "%s"  name
            copy_span(slot + sj, o + lj + 2u + ndj, cj, sub);                   // "%s"  sequence
            if (!fasta) copy_span(slot + qj, o + lj + 2u + ndj + cj + 3u, mj, sub);  // "%s"  quality line as read
        }
    }
}

uint64_t sample_tiles(uint32_t nl_cap) { return (uint64_t)(nl_cap / 4u) / kSmpTile + 1; }

// d_status: the look-back words of this pass (sample_tiles of them), zeroed here; d_state: as k_text_lines left it
hipError_t launch_sample_select(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last,
                                uint32_t carry_cap, uint32_t mode, uint32_t fasta, uint32_t seed_add, uint32_t threshold,
                                const uint64_t *d_picks, uint32_t n_picks, uint64_t ordinal0, uint32_t nl_cap, uint64_t *d_off,
                                uint64_t *d_keep, u64 *d_status, uint32_t *d_state, hipStream_t st)
{
    const uint64_t ts = sample_tiles(nl_cap);
    hipError_t e = hipMemsetAsync(d_status, 0, ts * sizeof(u64), st);
    if (e != hipSuccess) return e;
    const SampleArgs a{mode, fasta, seed_add, threshold, d_picks, n_picks, ordinal0};
    hipLaunchKernelGGL(k_sample_select, dim3((unsigned)ts), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, end, last, carry_cap, a,
                       d_off, d_keep, d_status, d_state);
    return hipGetLastError();
}

hipError_t launch_sample_write(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, const uint64_t *d_off,
                               const uint64_t *d_keep, uint32_t n_kept, uint32_t n, uint32_t n_lines, uint32_t unterminated,
                               uint64_t ordinal0, uint32_t fasta, uint8_t *d_out, int n_cu, hipStream_t st)
{
    if (n_kept == 0) return hipSuccess;
    uint64_t want = ((uint64_t)n_kept + kTxtThreads - 1) / kTxtThreads;
    const uint64_t cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_sample_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, d_off,
                       d_keep, n_kept, n, n_lines, unterminated, ordinal0, fasta, d_out);
    return hipGetLastError();
}

}  // namespace hpn
