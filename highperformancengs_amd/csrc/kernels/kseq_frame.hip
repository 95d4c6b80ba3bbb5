// kseq_frame.hip -- gfx950 kernels of hpn_kseq_*: klib's kseq_read as map_kseq.cpp and kbtree_kseq.c call it (a NEW kseq_t for
// every record), on the device, behind the line index of fastq_text.hip (docs/kernels/kseq.md).
//
// Two shapes are framed here; everything else raises HPN_TEXT_KSEQ and is read on the host (host/kseq_read.hpp).
//
//   FASTQ   four lines per record.  k_kseq_fq_recs, one thread per record: the four conditions, the header's split.
//   FASTA   every line that starts with '>' opens a BLOCK.  The new kseq_t has forgotten that the sequence loop consumed the
//           next block's '>', so kseq_read looks for the next '>' or '@' at any byte behind it: the blocks 0, 2, 4, ... are the
//           records, the blocks 1, 3, 5, ... are skipped and must hold no '>' or '@' behind their first byte.
//             k_kseq_fa_lines  per line: opens a block?  what it adds to the joined sequence (below)?  is it empty?
//             three scans      block of every line; offset of every line's bytes in the stream of joined bytes; non-empty lines
//             k_kseq_fa_heads  the header line of every block
//             k_kseq_fa_mark   the '>' / '@' search in the skipped blocks; the one line per record the '\r' rule spares
//             k_kseq_fa_recs   per record: the header's split, the joined length, the bounds
//             k_kseq_fa_copy   16 lanes per line: its bytes to their place in the record's joined sequence
//   both    a scan of the records' sizes, then k_kseq_put, 16 lanes per record: "name comment\n" ("(null)" for the comment
//           kseq_read leaves NULL), for FASTQ the sequence and the quality, and the record's SortDesc (sort_desc.hpp), so that
//           the refinement sort of fastq_sort.hip and a writer like k_sort_write run over the normalised store as they are.
//
// The '\r' rule in parallel.  ks_getuntil2 drops a trailing '\r' after every appended line when the ACCUMULATED length is above
// 1.  A line adds its length, minus one when it ends in '\r' -- except where the accumulated length is 1 after it: a line that is
// "\r" alone, appended to nothing.  Lines in front of it in the record then added nothing, and only empty lines add nothing, so it
// is the record's FIRST NON-EMPTY line and there is at most one per record.  So a line's tentative share t is its length minus its
// trailing '\r' (0 for a lone "\r"), the scan of t gives every line its offset, a scan of "non-empty" finds each record's first
// non-empty line, and where that one is a lone "\r" it is written at offset 0 and x = 1 is added to the offset of the record's
// later lines and to its length.  That is exact: every other line sees an accumulated length of at least 2 after its append.
//
// Bound: HBM -- the stream is read once by the line index, its kept bytes once more by the copies, and written once.
// All stores are vector stores in plain C++.
#include "sort_desc.hpp"
#include "text_common.hpp"

namespace hpn {

constexpr uint32_t kKseqNull = 0xffffffffu;   // KseqRec::com_len of a comment kseq_read leaves NULL
constexpr uint32_t kKseqMax = 65535u;         // the longest header line, joined sequence and "name comment" a descriptor holds
constexpr uint32_t kKseqFlag = 256u;          // HPN_TEXT_KSEQ (include/hpngs.h)

// what k_kseq_put needs of a record: offsets into the slot
struct KseqRec {
    uint32_t name, name_len, com, com_len, seq, slen, qual, qlen;
};

// the arrays over a chunk's lines (FASTA)
struct KseqLines {
    uint32_t *hdr, *t, *ne;     // opens a block; tentative share of the joined sequence; a non-empty sequence line
    uint32_t *hid, *P, *NE;     // their exclusive scans (n + 1 entries)
    uint32_t *hline;            // block -> its header line; hline[blocks] = lines
    uint32_t *x;                // record -> 1: its first non-empty line is a lone "\r", which stays
};

__device__ __forceinline__ bool kseq_space(uint8_t b) { return b == ' ' || (b >= 9u && b <= 13u); }   // isspace in the C locale

// The header's text p[0, len) behind its '>' or '@': the name up to the first isspace byte; the rest of the line behind that
// byte is the comment, NULL when the name ends the line.
__device__ __forceinline__ void kseq_header(const uint8_t *__restrict__ slot, uint32_t p, uint32_t len, KseqRec &x)
{
    uint32_t i = 0;
    while (i < len && !kseq_space(slot[p + i])) ++i;
    x.name = p, x.name_len = i;
    if (i == len) {
        x.com = p, x.com_len = kKseqNull;
        return;
    }
    uint32_t c = len - i - 1u;
    if (c > 1u && slot[p + len - 1u] == '\r') --c;
    x.com = p + i + 1u, x.com_len = c;
}

__device__ __forceinline__ uint32_t kseq_header_out(const KseqRec &x) { return x.name_len + 1u + (x.com_len == kKseqNull ? 6u : x.com_len); }

// ---- FASTQ shape --------------------------------------------------------------------------------------------------

// n_lines: the chunk's lines (with `last`, a final line without '\n' is closed by a virtual one at `end`).  Launched over
// n_lines / 4 records.  rsize[r]: the record's bytes in the normalised store.
__global__ __launch_bounds__(kTxtThreads) void k_kseq_fq_recs(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl,
                                                              uint32_t begin, uint32_t end, int last, uint32_t n_lines,
                                                              KseqRec *__restrict__ rec, uint32_t *__restrict__ rsize,
                                                              uint32_t *__restrict__ st)
{
    const uint32_t n = n_lines >> 2;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[kTsRecs] = n;
        uint32_t consumed = n ? nl[4u * n - 1u] + 1u : begin;
        if (consumed > end) consumed = end;   // the virtual newline
        if (last && end - consumed) atomicOr(&st[kTsFlags], kKseqFlag);   // a line count that 4 does not divide
        st[kTsConsumed] = consumed;
    }
    const uint32_t r = blockIdx.x * kTxtThreads + threadIdx.x;
    if (r >= n) return;
    u32 e;
    __builtin_memcpy(&e, nl + 4u * r, 16);
    const uint32_t p0 = r ? nl[4u * r - 1u] + 1u : begin;
    const uint32_t l0 = e[0] - p0, l1 = e[1] - e[0] - 1u, l2 = e[2] - e[1] - 1u, l3 = e[3] - e[2] - 1u;
    bool ok = l0 >= 1u && l1 >= 1u && l2 >= 1u && l0 - 1u <= kKseqMax && l1 <= kKseqMax;
    uint32_t s = 0, q = 0;
    KseqRec x = {};
    if (ok) {
        const uint8_t b1 = slot[e[0] + 1u];
        ok = slot[p0] == '@' && b1 != '>' && b1 != '+' && b1 != '@' && slot[e[1] + 1u] == '+';
        s = l1 - ((l1 > 1u && slot[e[1] - 1u] == '\r') ? 1u : 0u);
        q = l3 - ((l3 > 1u && slot[e[3] - 1u] == '\r') ? 1u : 0u);
        ok = ok && s == q;
    }
    if (ok) {
        kseq_header(slot, p0 + 1u, l0 - 1u, x);
        ok = kseq_header_out(x) <= kKseqMax;
    }
    if (!ok) {
        atomicOr(&st[kTsFlags], kKseqFlag);
        rsize[r] = 0u;
        return;
    }
    x.seq = e[0] + 1u, x.slen = s, x.qual = e[2] + 1u, x.qlen = q;
    rec[r] = x;
    rsize[r] = kseq_header_out(x) + 1u + s + 1u + q;
}

// ---- FASTA shape --------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t line_start(const uint32_t *__restrict__ nl, uint32_t i, uint32_t begin) { return i ? nl[i - 1u] + 1u : begin; }

// the blocks that are framed now: all of them at the stream's end; else an even number, and not the last one seen (whether
// it is complete only the next header tells)
__device__ __forceinline__ uint32_t fa_blocks(uint32_t H, int last) { return last ? H : (H ? (H - 1u) & ~1u : 0u); }

__global__ __launch_bounds__(256) void k_kseq_fa_lines(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl, uint32_t begin,
                                                       uint32_t n_lines, KseqLines a, uint32_t *__restrict__ st)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_lines) return;
    const uint32_t s = line_start(nl, i, begin), e = nl[i], len = e - s;
    const uint8_t b0 = len ? slot[s] : (uint8_t)0;
    const bool hdr = b0 == '>';
    const bool cr = len && slot[e - 1u] == '\r';
    uint32_t f = 0;
    if (b0 == '@' || b0 == '+') f = kKseqFlag;                                   // a FASTQ record, or one inside a FASTA file
    if (i == 0u && !hdr) f = kKseqFlag;                                          // (every chunk starts where a record starts)
    if (i == n_lines - 1u && st[kTsUnterminated] && (hdr || (len == 1u && cr)))   // the stream's end cuts a header, or leaves a line
        f = kKseqFlag;                                                            // of one '\r', which ks_getuntil2 then never sees
    if (f) atomicOr(&st[kTsFlags], f);
    a.hdr[i] = hdr ? 1u : 0u;
    a.ne[i] = !hdr && len ? 1u : 0u;
    a.t[i] = hdr || (len == 1u && cr) ? 0u : len - (cr ? 1u : 0u);
}

__global__ __launch_bounds__(256) void k_kseq_fa_heads(uint32_t n_lines, KseqLines a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) a.hline[a.hid[n_lines]] = n_lines;
    if (i < n_lines && a.hdr[i]) a.hline[a.hid[i]] = i;
}

// x: zeroed by the launcher
__global__ __launch_bounds__(256) void k_kseq_fa_mark(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl, uint32_t begin,
                                                      int last, uint32_t n_lines, KseqLines a, uint32_t *__restrict__ st)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_lines) return;
    const uint32_t R = fa_blocks(a.hid[n_lines], last);
    const uint32_t hdr = a.hdr[i];
    const uint32_t b = a.hid[i] + hdr - 1u;   // the line's block (line 0 opens block 0, or the chunk is flagged)
    if (b >= R) return;
    const uint32_t s = line_start(nl, i, begin), e = nl[i];
    if (b & 1u) {   // a skipped block: kseq_read stops at a '>' or '@' anywhere in it
        bool hit = false;
        for (uint32_t p = s + hdr; p < e; ++p) hit |= slot[p] == '>' || slot[p] == '@';
        if (hit) atomicOr(&st[kTsFlags], kKseqFlag);
        return;
    }
    if (!hdr && a.ne[i] && a.NE[i] == a.NE[a.hline[b]] && e - s == 1u && slot[s] == '\r') a.x[b >> 1] = 1u;
}

// Launched over an upper bound of records, (n_lines + 1) / 2; rsize is written for all of them (0 behind the last record).
__global__ __launch_bounds__(256) void k_kseq_fa_recs(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl, uint32_t begin,
                                                      uint32_t end, int last, uint32_t n_lines, KseqLines a, KseqRec *__restrict__ rec,
                                                      uint32_t *__restrict__ rsize, uint32_t *__restrict__ st)
{
    const uint32_t H = a.hid[n_lines], R = fa_blocks(H, last), K = (R + 1u) >> 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[kTsRecs] = K;
        st[kTsConsumed] = last ? end : (H ? line_start(nl, a.hline[R], begin) : begin);
        // the record that stays unframed (block R, an even one) is already too long: say so now, not when its end arrives
        if (!last && H && a.P[a.hline[R + 1u]] - a.P[a.hline[R]] > kKseqMax) atomicOr(&st[kTsFlags], kKseqFlag);
    }
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (n_lines + 1u) >> 1) return;
    if (k >= K) {
        rsize[k] = 0u;
        return;
    }
    const uint32_t hl = a.hline[2u * k], next = a.hline[2u * k + 1u];
    const uint32_t s = line_start(nl, hl, begin), len = nl[hl] - s - 1u;   // the header's text behind '>'
    const uint32_t T = a.P[next] - a.P[hl] + a.x[k];
    KseqRec x = {};
    if (len > kKseqMax || T > kKseqMax) {
        atomicOr(&st[kTsFlags], kKseqFlag);
        rsize[k] = 0u;
        return;
    }
    kseq_header(slot, s + 1u, len, x);
    if (kseq_header_out(x) > kKseqMax) {
        atomicOr(&st[kTsFlags], kKseqFlag);
        rsize[k] = 0u;
        return;
    }
    x.slen = T;
    rec[k] = x;
    rsize[k] = kseq_header_out(x) + 1u + T + 1u;
}

// 16 lanes per line.  dst: where the chunk's first record goes in the normalised store.
__global__ __launch_bounds__(kTxtThreads) void k_kseq_fa_copy(const uint8_t *__restrict__ slot, const uint32_t *__restrict__ nl,
                                                              uint32_t begin, int last, uint32_t n_lines, KseqLines a,
                                                              const KseqRec *__restrict__ rec, const uint64_t *__restrict__ roff,
                                                              uint8_t *__restrict__ dst)
{
    const uint32_t groups = gridDim.x * (kTxtThreads / 16u);
    const int sub = (int)(threadIdx.x & 15u);
    const uint32_t R = fa_blocks(a.hid[n_lines], last);
    for (uint32_t i = blockIdx.x * (kTxtThreads / 16u) + (threadIdx.x >> 4); i < n_lines; i += groups) {
        if (a.hdr[i]) continue;
        const uint32_t b = a.hid[i] - 1u;
        if (b >= R || (b & 1u)) continue;
        const uint32_t k = b >> 1, hl = a.hline[b], s = line_start(nl, i, begin);
        const KseqRec x = rec[k];
        uint8_t *o = dst + roff[k] + kseq_header_out(x) + 1u;
        const uint32_t t = a.t[i];
        if (t) copy_span(slot + s, o + (a.P[i] - a.P[hl]) + a.x[k], t, sub);
        else if (a.ne[i] && a.NE[i] == a.NE[hl] && sub == 0) o[0] = '\r';   // (non-empty with t = 0: a lone "\r"; the first one stays)
    }
}

// ---- both shapes: the records into the normalised store ------------------------------------------------------------

// norm: the normalised store's byte 0; origin: where this chunk's first record goes.  n comes from st[kTsRecs].
__global__ __launch_bounds__(kTxtThreads) void k_kseq_put(const uint8_t *__restrict__ slot, const KseqRec *__restrict__ rec,
                                                          const uint64_t *__restrict__ roff, const uint32_t *__restrict__ st, int fastq,
                                                          uint8_t *__restrict__ norm, u64 origin, SortDesc *__restrict__ desc)
{
    const uint32_t n = st[kTsRecs];
    const uint32_t groups = gridDim.x * (kTxtThreads / 16u);
    const int sub = (int)(threadIdx.x & 15u);
    for (uint32_t k = blockIdx.x * (kTxtThreads / 16u) + (threadIdx.x >> 4); k < n; k += groups) {
        const KseqRec x = rec[k];
        const u64 at = origin + roff[k];
        uint8_t *o = norm + at;
        const uint32_t hout = kseq_header_out(x);
        copy_span(slot + x.name, o, x.name_len, sub);
        if (x.com_len != kKseqNull) copy_span(slot + x.com, o + x.name_len + 1u, x.com_len, sub);
        if (fastq) {
            copy_span(slot + x.seq, o + hout + 1u, x.slen, sub);
            copy_span(slot + x.qual, o + hout + 1u + x.slen + 1u, x.qlen, sub);
        }
        if (sub == 0) {
            uint8_t *c = o + x.name_len;
            c[0] = ' ';
            if (x.com_len == kKseqNull) c[1] = '(', c[2] = 'n', c[3] = 'u', c[4] = 'l', c[5] = 'l', c[6] = ')';
            o[hout] = '\n';
            o[hout + 1u + x.slen] = '\n';
            SortDesc d;
            d.off = at;
            d.nlen = (uint16_t)hout, d.slen = (uint16_t)x.slen, d.qlen = (uint16_t)x.qlen;
            d.qrel = (uint16_t)(hout + 1u + x.slen + 1u);   // (mod 2^16: k_kseq_write takes the quality's place from nlen and slen)
            desc[k] = d;
        }
    }
}

// ---- _finish: the first record of every run of equal sequences, and the output -------------------------------------

// do the `len` bytes at a and b differ?  (span_differs of fastq_sort.hip)
__device__ __forceinline__ bool kseq_differs(const uint8_t *a, const uint8_t *b, uint32_t len)
{
    for (uint32_t o = 0; o < len; o += 16u) {
        u32 x, y;
        __builtin_memcpy(&x, a + o, 16);
        __builtin_memcpy(&y, b + o, 16);
        const uint32_t rem = len - o;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            uint32_t df = x[q] ^ y[q];
            if (rem < 4u * q + 4u) df = rem > 4u * q ? df & (0xffffffffu >> (8u * (4u * q + 4u - rem))) : 0u;
            if (df) return true;
        }
    }
    return false;
}

// head[q]: the q-th record of the order opens a run -- its sequence differs from its predecessor's in length or in a byte.
// The sorts are stable: a run's head is its earliest record.
__global__ __launch_bounds__(256) void k_kseq_heads(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc,
                                                    const uint32_t *__restrict__ order, uint32_t n, uint32_t *__restrict__ head)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    if (q == 0u) {
        head[0] = 1u;
        return;
    }
    const SortDesc a = desc[order[q]], b = desc[order[q - 1u]];
    head[q] = a.slen != b.slen || kseq_differs(text + a.off + a.nlen + 1u, text + b.off + b.nlen + 1u, a.slen) ? 1u : 0u;
}

// info[0]: the smallest ordinal of a record whose sequence length is not the first record's (the launcher sets it to ~0)
__global__ __launch_bounds__(256) void k_kseq_lens(const SortDesc *__restrict__ desc, uint32_t n, uint32_t *__restrict__ info)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && desc[i].slen != desc[0].slen) atomicMin(info, i);
}

// at: the exclusive scan of head.  pick[at[q]] = the record, size[at[q]] = its bytes in the output.
__global__ __launch_bounds__(256) void k_kseq_pick(const SortDesc *__restrict__ desc, const uint32_t *__restrict__ order,
                                                   const uint32_t *__restrict__ head, const uint32_t *__restrict__ at, uint32_t n, int fastq,
                                                   uint32_t *__restrict__ pick, uint32_t *__restrict__ size)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n || !head[q]) return;
    const uint32_t r = order[q];
    const SortDesc d = desc[r];
    pick[at[q]] = r;
    size[at[q]] = (uint32_t)d.nlen + 1u + d.slen + 3u + (fastq ? (uint32_t)d.qlen : 6u) + 1u;   // "%s %s\n%s\n+\n%s\n"
}

// k_sort_write's plan -- a lane per record for the fixed bytes, 16 lanes per record for the spans -- over the picked records
__global__ __launch_bounds__(kTxtThreads) void k_kseq_write(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc,
                                                            const uint32_t *__restrict__ pick, const uint64_t *__restrict__ off, uint32_t n,
                                                            int fastq, uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, dst = 0;
        uint32_t nlen = 0, slen = 0, qlen = 0;
        if (k < n) {
            const SortDesc d = desc[pick[k]];
            src = d.off, dst = off[k];
            nlen = d.nlen, slen = d.slen, qlen = d.qlen;
            uint8_t *o = out + dst + nlen;
            o[0] = '\n';
            o += 1u + slen;
            o[0] = '\n', o[1] = '+', o[2] = '\n';
            if (fastq) {
                o[3u + qlen] = '\n';
            } else {
                o[3] = '(', o[4] = 'n', o[5] = 'u', o[6] = 'l', o[7] = 'l', o[8] = ')', o[9] = '\n';
            }
        }
#pragma unroll 2
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t nj = __shfl(nlen, j, kWave), cj = __shfl(slen, j, kWave), mj = __shfl(qlen, j, kWave);
            if (k0 + (uint32_t)j >= n) continue;
            uint8_t *o = out + dj;
            copy_span(text + sj, o, nj, sub);
            copy_span(text + sj + nj + 1u, o + nj + 1u, cj, sub);
            if (fastq) copy_span(text + sj + nj + 1u + cj + 1u, o + nj + 1u + cj + 3u, mj, sub);   // (the quality lies behind the sequence's '\n')
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned kblocks(uint32_t n, uint32_t per) { return n ? (n + per - 1u) / per : 1u; }
static inline unsigned kgroups(uint32_t n, int n_cu)   // 16 lanes per item
{
    const unsigned want = kblocks(n, kTxtThreads / 16u), cap = (unsigned)n_cu * 8u;
    return want < cap ? want : cap;
}

hipError_t launch_kseq_fq_recs(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint32_t n_lines,
                               void *d_rec, uint32_t *d_rsize, uint32_t *d_state, hipStream_t st)
{
    hipLaunchKernelGGL(k_kseq_fq_recs, dim3(kblocks(n_lines / 4u, kTxtThreads)), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, end, last,
                       n_lines, (KseqRec *)d_rec, d_rsize, d_state);
    return hipGetLastError();
}

hipError_t launch_kseq_fa_lines(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t n_lines, const KseqLines &a,
                                uint32_t *d_state, hipStream_t st)
{
    hipLaunchKernelGGL(k_kseq_fa_lines, dim3(kblocks(n_lines, 256u)), dim3(256), 0, st, d_slot, d_nl, begin, n_lines, a, d_state);
    return hipGetLastError();
}

// behind the three scans
hipError_t launch_kseq_fa_recs(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint32_t n_lines,
                               const KseqLines &a, void *d_rec, uint32_t *d_rsize, uint32_t *d_state, hipStream_t st)
{
    const uint32_t kmax = (n_lines + 1u) / 2u;
    hipError_t e = hipMemsetAsync(a.x, 0, ((size_t)kmax + 1u) * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_kseq_fa_heads, dim3(kblocks(n_lines, 256u)), dim3(256), 0, st, n_lines, a);
    hipLaunchKernelGGL(k_kseq_fa_mark, dim3(kblocks(n_lines, 256u)), dim3(256), 0, st, d_slot, d_nl, begin, last, n_lines, a, d_state);
    hipLaunchKernelGGL(k_kseq_fa_recs, dim3(kblocks(kmax, 256u)), dim3(256), 0, st, d_slot, d_nl, begin, end, last, n_lines, a,
                       (KseqRec *)d_rec, d_rsize, d_state);
    return hipGetLastError();
}

hipError_t launch_kseq_fa_copy(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, int last, uint32_t n_lines, const KseqLines &a,
                               const void *d_rec, const uint64_t *d_roff, uint8_t *d_dst, int n_cu, hipStream_t st)
{
    if (!n_lines) return hipSuccess;
    hipLaunchKernelGGL(k_kseq_fa_copy, dim3(kgroups(n_lines, n_cu)), dim3(kTxtThreads), 0, st, d_slot, d_nl, begin, last, n_lines, a,
                       (const KseqRec *)d_rec, d_roff, d_dst);
    return hipGetLastError();
}

// max_records: an upper bound of st[kTsRecs]
hipError_t launch_kseq_put(const uint8_t *d_slot, const void *d_rec, const uint64_t *d_roff, const uint32_t *d_state, uint32_t max_records,
                           int fastq, uint8_t *d_norm, uint64_t origin, void *d_desc, int n_cu, hipStream_t st)
{
    if (!max_records) return hipSuccess;
    hipLaunchKernelGGL(k_kseq_put, dim3(kgroups(max_records, n_cu)), dim3(kTxtThreads), 0, st, d_slot, (const KseqRec *)d_rec, d_roff,
                       d_state, fastq, d_norm, (u64)origin, (SortDesc *)d_desc);
    return hipGetLastError();
}

hipError_t launch_kseq_heads(const uint8_t *d_text, const void *d_desc, const uint32_t *d_order, uint32_t n, uint32_t *d_head,
                             uint32_t *d_info, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_info, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess || !n) return e;
    hipLaunchKernelGGL(k_kseq_heads, dim3(kblocks(n, 256u)), dim3(256), 0, st, d_text, (const SortDesc *)d_desc, d_order, n, d_head);
    hipLaunchKernelGGL(k_kseq_lens, dim3(kblocks(n, 256u)), dim3(256), 0, st, (const SortDesc *)d_desc, n, d_info);
    return hipGetLastError();
}

hipError_t launch_kseq_pick(const void *d_desc, const uint32_t *d_order, const uint32_t *d_head, const uint32_t *d_at, uint32_t n, int fastq,
                            uint32_t *d_pick, uint32_t *d_size, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_kseq_pick, dim3(kblocks(n, 256u)), dim3(256), 0, st, (const SortDesc *)d_desc, d_order, d_head, d_at, n, fastq, d_pick,
                       d_size);
    return hipGetLastError();
}

hipError_t launch_kseq_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_pick, const uint64_t *d_off, uint32_t n, int fastq,
                             uint8_t *d_out, int n_cu, hipStream_t st)
{
    if (!n) return hipSuccess;
    const unsigned want = kblocks(n, kTxtThreads), cap = (unsigned)n_cu * 8u;
    hipLaunchKernelGGL(k_kseq_write, dim3(want < cap ? want : cap), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc, d_pick, d_off, n,
                       fastq, d_out);
    return hipGetLastError();
}

}  // namespace hpn
