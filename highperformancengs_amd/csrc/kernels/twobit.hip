// twobit.hip -- gfx950 kernels of hpn_twobit_* (fastq2twobit.c and twoBit2seq.c with the packing of twoBit.h on the device).
//
// The reference pushes every record on the front of a list and dumps the list from its head: the output holds the records in
// REVERSE input order, a 2-byte header -- (uint8_t)strlen and (uint8_t)packed length of the first record WRITTEN, the input's
// last -- and then, per record, (len + 3) >> 2 bytes: four bases per byte, the first base in the top bits, T / U / anything
// else 0, C 1, A 2, G 3 in either case, the tail of the last byte 0.  Records of different lengths are simply concatenated.
// The inverse reads that header and cuts the body into records of packedLen bytes, of which it prints seqlen bases and '\n'.
//
//   k_pack_sizes     size[q] = packed bytes of record N-1-q (the stream lies in the device store, hpn_store.hpp, with the
//                    16-byte SortDesc of k_sort_frame per record); uniq_scan64 turns them into offsets.
//   k_pack_write     16 lanes per record (the team shape of k_sort_write): a lane turns 16 sequence bytes -- one 16-byte load,
//                    any alignment -- into 4 output bytes, any alignment.  The last load of a record is moved back so that it
//                    ends with the sequence (copy_span's clamp) and its bytes are shifted down; a sequence shorter than 16 is
//                    read by bytes.  No load reaches behind the sequence's last byte.  Output position 0's team writes the header.
//                    A sequence byte >= 0x80 (the reference indexes its table with a signed char there) is reported: one
//                    atomicMin of the smallest such record ordinal per lane that saw one.
//   k_twobit_unpack  stateless, fixed strides: output byte p is column p % (seqlen + 1) of record p / (seqlen + 1); a lane makes
//                    one ALIGNED 16-byte store of the flat output, stepping (record, column) from one division; the bytes in
//                    front of the first aligned vector and behind the last go out bytewise.  Record bytes behind packedLen
//                    read as 0 (the reference's zeroed buffer).
//
// Bound: HBM.  Pack reads the sequence bytes once (and 16 + 8 bytes of descriptor and offset per record) and writes a quarter
// of them; unpack reads a quarter of what it writes (docs/kernels/twobit.md).
#include "sort_desc.hpp"
#include "text_common.hpp"

namespace hpn {

__global__ __launch_bounds__(256) void k_pack_sizes(const SortDesc *__restrict__ desc, uint32_t n, uint32_t *__restrict__ size)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    size[q] = ((uint32_t)desc[n - 1u - q].slen + 3u) >> 2;
}

// four bases of one little-endian word (the first base is the lowest byte) -> one byte, the first base in the top bits
__device__ __forceinline__ uint32_t pack4(uint32_t w)
{
    uint32_t out = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t c = ((w >> (8u * b)) & 0xffu) | 0x20u;   // folds the case: exactly 'C' and 'c' become 'c', ...
        const uint32_t code = (c == 'c' ? 1u : 0u) + (c == 'a' ? 2u : 0u) + (c == 'g' ? 3u : 0u);
        out = (out << 2) | code;
    }
    return out;
}

// One record by 16 lanes: slen sequence bytes at src -> (slen + 3) >> 2 bytes at dst.  true: this lane saw a byte >= 0x80.
__device__ __forceinline__ bool pack_span(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t slen, int sub)
{
    const uint32_t plen = (slen + 3u) >> 2;
    bool high = false;
    for (uint32_t o = 16u * (uint32_t)sub; o < slen; o += 256u) {
        const uint32_t rem = slen - o;   // sequence bytes from o on
        u64 v[2] = {0ull, 0ull};         // bytes behind the sequence's end stay 0: code 0, the padding
        if (rem >= 16u) {
            __builtin_memcpy(v, src + o, 16);
        } else if (slen >= 16u) {
            __builtin_memcpy(v, src + slen - 16u, 16);   // ends with the sequence; its first 16 - rem bytes belong to the lane before
            const uint32_t s = 8u * (16u - rem);
            if (s >= 64u) v[0] = v[1] >> (s - 64u), v[1] = 0ull;
            else v[0] = (v[0] >> s) | (v[1] << (64u - s)), v[1] >>= s;
        } else {
            for (uint32_t b = 0; b < rem; ++b) v[b >> 3] |= (u64)src[b] << (8u * (b & 7u));   // (o is 0: the whole sequence)
        }
        high |= ((v[0] | v[1]) & 0x8080808080808080ull) != 0ull;
        const uint32_t w = pack4((uint32_t)v[0]) | (pack4((uint32_t)(v[0] >> 32)) << 8) | (pack4((uint32_t)v[1]) << 16) |
                           (pack4((uint32_t)(v[1] >> 32)) << 24);
        uint8_t *p = dst + (o >> 2);
        const uint32_t left = plen - (o >> 2);   // output bytes from here on
        if (left >= 4u) {
            __builtin_memcpy(p, &w, 4);
        } else {
            for (uint32_t b = 0; b < left; ++b) p[b] = (uint8_t)(w >> (8u * b));
        }
    }
    return high;
}

// off: the exclusive scan of k_pack_sizes; out: 2 + off[n] bytes; bad: one word, 0xffffffff before the launch
__global__ __launch_bounds__(kTxtThreads) void k_pack_write(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc,
                                                            const uint64_t *__restrict__ off, uint32_t n, uint8_t *__restrict__ out,
                                                            uint32_t *__restrict__ bad)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    uint32_t worst = 0xffffffffu;   // the smallest ordinal in which this lane saw a high byte
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;   // output position: record n - 1 - k
        u64 src = 0, dst = 0;
        uint32_t slen = 0;
        if (k < n) {
            const SortDesc d = desc[n - 1u - k];
            src = d.off + d.nlen + 1u, dst = 2u + off[k], slen = d.slen;
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t cj = __shfl(slen, j, kWave);
            const uint32_t kj = k0 + (uint32_t)j;
            if (kj >= n) continue;
            if (kj == 0u && sub == 0) out[0] = (uint8_t)cj, out[1] = (uint8_t)((cj + 3u) >> 2);   // the header: both modulo 256
            if (pack_span(text + sj, out + dj, cj, sub)) worst = min(worst, n - 1u - kj);
        }
    }
    if (worst != 0xffffffffu) atomicMin(bad, worst);
}

// `count` <= 16 bytes of the flat output from byte p on, little-endian in v[0], v[1]
__device__ __forceinline__ void unpack16(const uint8_t *__restrict__ packed, uint32_t seqlen, uint32_t plen, u64 p, uint32_t count, u64 v[2])
{
    const u64 stride = (u64)seqlen + 1u;
    u64 rec = p / stride;
    uint32_t col = (uint32_t)(p - rec * stride);
    const uint8_t *r = packed + rec * plen;
    uint32_t cur = (col < seqlen && (col >> 2) < plen) ? r[col >> 2] : 0u;   // the record byte that holds column col
    v[0] = v[1] = 0ull;
#pragma unroll
    for (uint32_t b = 0; b < 16u; ++b) {
        if (b < count) {
            uint32_t ch;
            if (col == seqlen) {
                ch = '\n';
                col = 0u, r += plen;
                cur = seqlen ? r[0] : 0u;   // the NEXT record's first byte (plen >= 1): the caller ends `count` in front of the output's last '\n'
            } else {
                ch = (0x47414354u >> (8u * ((cur >> (6u - 2u * (col & 3u))) & 3u))) & 0xffu;   // "TCAG"
                ++col;
                if ((col & 3u) == 0u && col < seqlen) cur = (col >> 2) < plen ? r[col >> 2] : 0u;
            }
            v[b >> 3] |= (u64)ch << (8u * (b & 7u));
        }
    }
}

// total = n_records * (seqlen + 1) bytes at out; head: bytes in front of the first 16-byte aligned address of out (< 16, <= total)
__global__ __launch_bounds__(256) void k_twobit_unpack(const uint8_t *__restrict__ packed, uint32_t seqlen, uint32_t plen, u64 total,
                                                       uint32_t head, uint8_t *__restrict__ out)
{
    const u64 nvec = (total - head) >> 4;
    const uint32_t tail = (uint32_t)((total - head) & 15u);
    u64 v[2];
    // items 0 .. nvec - 1: the aligned vectors; item nvec: the bytes in front of them; item nvec + 1: the bytes behind them
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < nvec + 2u; i += (u64)gridDim.x * 256u) {
        const bool vec = i < nvec;
        const u64 p = vec ? head + 16u * i : (i == nvec ? 0ull : head + 16u * nvec);
        const uint32_t count = vec ? 16u : (i == nvec ? head : tail);
        if (!count) continue;
        // the step behind a '\n' loads the next record's first byte, and behind the last record there is none
        const bool ends = p + count == total;
        unpack16(packed, seqlen, plen, p, ends ? count - 1u : count, v);
        if (ends) v[(count - 1u) >> 3] |= (u64)'\n' << (8u * ((count - 1u) & 7u));
        if (vec) {
            u64 *q = (u64 *)__builtin_assume_aligned(out + p, 16);
            __builtin_memcpy(q, v, 16);
        } else {
            for (uint32_t b = 0; b < count; ++b) out[p + b] = (uint8_t)(v[b >> 3] >> (8u * (b & 7u)));
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

hipError_t launch_pack_sizes(const void *d_desc, uint32_t n, uint32_t *d_size, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack_sizes, dim3((n + 255u) / 256u), dim3(256), 0, st, (const SortDesc *)d_desc, n, d_size);
    return hipGetLastError();
}

// d_bad: set to 0xffffffff here
hipError_t launch_pack_write(const uint8_t *d_text, const void *d_desc, const uint64_t *d_off, uint32_t n, uint8_t *d_out, uint32_t *d_bad,
                             int n_cu, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess || n == 0) return e;
    const uint64_t want = ((uint64_t)n + kTxtThreads - 1) / kTxtThreads, cap = (uint64_t)n_cu * 8;
    hipLaunchKernelGGL(k_pack_write, dim3((unsigned)(want < cap ? want : cap)), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc, d_off,
                       n, d_out, d_bad);
    return hipGetLastError();
}

// packed_len >= 1, n_records >= 1; d_out holds n_records * (seq_len + 1) bytes
hipError_t launch_twobit_unpack(const uint8_t *d_packed, uint32_t seq_len, uint32_t packed_len, uint64_t n_records, uint8_t *d_out, int n_cu,
                                hipStream_t st)
{
    const uint64_t total = n_records * ((uint64_t)seq_len + 1u);
    uint32_t head = (uint32_t)((16u - ((uintptr_t)d_out & 15u)) & 15u);
    if (head > total) head = (uint32_t)total;
    const uint64_t items = ((total - head) >> 4) + 2u, want = (items + 255u) / 256u, cap = (uint64_t)n_cu * 32;
    hipLaunchKernelGGL(k_twobit_unpack, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, d_packed, seq_len, packed_len,
                       (u64)total, head, d_out);
    return hipGetLastError();
}

}  // namespace hpn
