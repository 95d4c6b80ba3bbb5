// mrle.hip -- gfx950 kernels of hpn_mrle_* (gzfastq_mrle.c: mrlec2 / mrled2 over the quality lines, and its two output streams).
//
// The codec knows six symbols, '#' 0, '/' 1, '7' 2, '<' 3, 'B' 4, 'F' 5.  Pass 1 sums per symbol, over its maximal runs of length
// L, L - 2 - (L - 1) / 255; the flag byte has bit s set where that sum is positive.  Pass 2 writes a run of a flagged symbol as
// the symbol, (L - 1) / 255 bytes 0xFF and the byte L - 255 * ((L - 1) / 255) - 1, every other run as its L bytes.  The packed
// file holds per record (uint8_t)size and the size bytes; the decoder, given the line's length, prints the line again.
//
//   k_mrle_sizes    16 lanes per record (the team shape of k_sort_write / k_pack_write), 16 quality bytes per lane and step, 256
//                   per team step.  A run's start is found against the byte in front of the lane's span (one byte load inside the
//                   line); the start of the run that is open where a lane begins comes from a prefix maximum of "last start in my
//                   span" over the team, carried over the steps, so that the lane that holds a run's LAST byte knows its length
//                   whatever it spans.  That lane adds L - 1 - (L - 1) / 255 and 1 run to two words of six 10-bit fields; the
//                   team sums both, savings = the difference, size = 1 + len - the flagged savings.  Writes 1 + size and len + 1
//                   for the two scans, and the flag byte.  A byte outside the six (classified by compares) is reported like
//                   k_pack_write's high byte: one atomicMin of the smallest such ordinal per lane that saw one.
//   k_mrle_write    the same walk; a byte's output position is the team-wide prefix sum of 1 for a byte of an unflagged symbol
//                   and of 2 + (L - 1) / 255 at a flagged run's LAST byte (0 inside it: the sum in front of the run's last byte
//                   is the sum in front of its first, and only the last byte's lane knows L).  Length byte, flag byte and tokens
//                   go out bytewise at any alignment.
//   k_mrle_decode   reads the ENCODED bytes and the line's length, never the store.  A token byte is a symbol or a count
//                   depending on what stands in front of it, which is a two-state machine (expect a symbol / expect a count):
//                   every lane composes its 16 bytes' transitions into one map of 2 bits, the team scans the maps, and each lane
//                   then knows the state it starts in -- no lane walks the whole record.  A second walk gives the decoded bytes
//                   per lane and the symbol of a token that is open across lanes (prefix sum, "last seen" scan); the third
//                   writes: short runs by their lane, runs of more than 8 bytes by the whole team, one at a time.  Every store
//                   is clamped to the line's length.
//   k_mrle_shared   one workgroup per 4,096-byte block of the shared descriptor's output (hpn_mrle.hip).  Block b of a stream
//                   leaves during the first call of record r that takes the stream's total beyond 4096 (b + 1): one binary search
//                   in that stream's offsets.  Within a record the text's calls stand in front of the packed stream's, so the
//                   blocks of the OTHER stream that left earlier are counted by one look at its offset of r (text block) or of
//                   r + 1 (packed block): the merge of the two monotone lists needs no second search.  The last workgroup copies
//                   the packed stream's remainder.
//
// No load reaches in front of or behind a quality line or a record's encoded bytes: the last 16-byte load of a span is moved back
// so that it ends with the span (copy_span's clamp), a span shorter than 16 is read by bytes.
//
// Bound: HBM for the sizes pass (reads the quality bytes once); the writers are bound by their bytewise stores
// (docs/kernels/mrle.md).
#include "sort_desc.hpp"
#include "text_common.hpp"

namespace hpn {

constexpr uint32_t kMrleBlock = 4096;   // glibc's buffer for a pipe or a regular file
constexpr uint32_t kNone = 0x100;       // no byte (in front of the line, behind it; no open token)

__device__ __forceinline__ uint32_t mrle_index(uint32_t c)
{
    return c == '#' ? 0u : c == '/' ? 1u : c == '7' ? 2u : c == '<' ? 3u : c == 'B' ? 4u : c == 'F' ? 5u : 6u;
}

__device__ __forceinline__ uint32_t byte_of(const u64 v[2], uint32_t b) { return (uint32_t)(((b & 8u) ? v[1] : v[0]) >> (8u * (b & 7u))) & 0xffu; }

// The lane's up to 16 bytes of the span [src, src + len) from byte o on, little-endian in v; returns how many (0: o is behind the span)
__device__ __forceinline__ uint32_t load_lane(const uint8_t *__restrict__ src, uint32_t len, uint32_t o, u64 v[2])
{
    v[0] = v[1] = 0ull;
    if (o >= len) return 0u;
    const uint32_t rem = len - o;
    if (rem >= 16u) {
        __builtin_memcpy(v, src + o, 16);
        return 16u;
    }
    if (len >= 16u) {
        __builtin_memcpy(v, src + len - 16u, 16);   // ends with the span; its first 16 - rem bytes belong to the lane before
        const uint32_t s = 8u * (16u - rem);
        if (s >= 64u) v[0] = v[1] >> (s - 64u), v[1] = 0ull;
        else v[0] = (v[0] >> s) | (v[1] << (64u - s)), v[1] >>= s;
    } else {
        for (uint32_t b = 0; b < rem; ++b) v[b >> 3] |= (u64)src[o + b] << (8u * (b & 7u));
    }
    return rem;
}

// What a lane knows of the runs in its span of a quality line: its bytes, the byte in front of them and behind them (kNone at the
// line's ends) and `start`, where the run begins that is open at the lane's first byte.
struct LaneRuns {
    u64 v[2];
    uint32_t o, cnt, prev, next;
    int32_t start;
};

// Called by all 16 lanes of a team, for every 256-byte step of the line; carry: -1 before the first step
__device__ __forceinline__ void lane_runs(const uint8_t *__restrict__ src, uint32_t len, uint32_t base, int sub, int32_t &carry, LaneRuns &r)
{
    r.o = base + 16u * (uint32_t)sub;
    r.cnt = load_lane(src, len, r.o, r.v);
    r.prev = (r.cnt && r.o) ? src[r.o - 1u] : kNone;
    r.next = (r.cnt && r.o + r.cnt < len) ? src[r.o + r.cnt] : kNone;
    int32_t last = -1;   // the last run start in this lane's span
    uint32_t p = r.prev;
#pragma unroll
    for (uint32_t b = 0; b < 16u; ++b) {
        if (b < r.cnt) {
            const uint32_t c = byte_of(r.v, b);
            if (c != p) last = (int32_t)(r.o + b);
            p = c;
        }
    }
    int32_t inc = last;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        const int32_t t = __shfl_up(inc, d, 16);
        if (sub >= d) inc = max(inc, t);
    }
    const int32_t ex = __shfl_up(inc, 1, 16);
    r.start = max(sub ? ex : -1, carry);
    carry = max(carry, __shfl(inc, 15, 16));
}

// the longest span (bytes) among the four teams of the wave: the step loops are uniform over the wave
__device__ __forceinline__ uint32_t wave_span(uint32_t len)
{
    len = max(len, (uint32_t)__shfl_xor(len, 16, kWave));
    return max(len, (uint32_t)__shfl_xor(len, 32, kWave));
}

// One line by 16 lanes.  A, R: six 10-bit fields, per symbol the sum of L - 1 - (L - 1) / 255 over its runs and the number of its
// runs (both at most 1022), summed over the team.  true: this lane saw a byte outside the six.
__device__ __forceinline__ bool line_savings(const uint8_t *__restrict__ src, uint32_t len, uint32_t steps, int sub, u64 &A, u64 &R)
{
    bool bad = false;
    int32_t carry = -1;
    A = R = 0ull;
    for (uint32_t base = 0; base < steps; base += 256u) {
        LaneRuns r;
        lane_runs(src, len, base, sub, carry, r);
        int32_t st = r.start;
        uint32_t p = r.prev;
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b) {
            if (b < r.cnt) {
                const uint32_t c = byte_of(r.v, b), pos = r.o + b;
                if (c != p) st = (int32_t)pos;
                const uint32_t nx = b + 1u < r.cnt ? byte_of(r.v, (b + 1u) & 15u) : r.next;
                if (c != nx) {   // the run's last byte
                    const uint32_t L = pos - (uint32_t)st + 1u, idx = mrle_index(c);
                    if (idx < 6u) A += (u64)(L - 1u - (L - 1u) / 255u) << (10u * idx), R += 1ull << (10u * idx);
                    else bad = true;
                }
                p = c;
            }
        }
    }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) A += __shfl_xor(A, d, 16), R += __shfl_xor(R, d, 16);
    return bad;
}

// psize[k] = 1 + encoded size, tsize[k] = len + 1, flag[k]; bad: one word, 0xffffffff before the launch
__global__ __launch_bounds__(kTxtThreads) void k_mrle_sizes(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc, uint32_t n,
                                                            uint32_t *__restrict__ psize, uint32_t *__restrict__ tsize, uint8_t *__restrict__ flag,
                                                            uint32_t *__restrict__ bad)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    uint32_t worst = 0xffffffffu;   // the smallest ordinal in which this lane saw a byte outside the six
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0;
        uint32_t qlen = 0;
        if (k < n) {
            const SortDesc d = desc[k];
            src = d.off + d.qrel, qlen = d.qlen;
        }
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave);
            const uint32_t kj = k0 + (uint32_t)j;
            const uint32_t qj = __shfl(qlen, j, kWave);
            const uint32_t mj = kj < n ? qj : 0u;   // a team without a record walks an empty line
            u64 A, R;
            if (line_savings(text + sj, mj, wave_span(mj), sub, A, R)) worst = min(worst, kj);
            if (kj < n && sub == 0) {
                uint32_t flags = 0, size = 1u + mj;
#pragma unroll
                for (uint32_t s = 0; s < 6u; ++s) {
                    const int32_t t = (int32_t)((A >> (10u * s)) & 1023u) - (int32_t)((R >> (10u * s)) & 1023u);
                    if (t > 0) flags |= 1u << s, size -= (uint32_t)t;
                }
                psize[kj] = 1u + size, tsize[kj] = mj + 1u, flag[kj] = (uint8_t)flags;
            }
        }
    }
    if (worst != 0xffffffffu) atomicMin(bad, worst);
}

// One line by 16 lanes: its tokens at dst.  cap: the token bytes k_mrle_sizes counted -- the walk is the same, so no store is ever
// refused; the test keeps a record inside its own bytes by construction.
__device__ __forceinline__ void line_encode(const uint8_t *__restrict__ src, uint32_t len, uint32_t steps, uint32_t flags, uint8_t *__restrict__ dst,
                                            uint32_t cap, int sub)
{
    int32_t carry = -1;
    uint32_t at = 0;   // token bytes written by the steps before
    for (uint32_t base = 0; base < steps; base += 256u) {
        LaneRuns r;
        lane_runs(src, len, base, sub, carry, r);
        uint32_t w = 0;
        for (int pass = 0; pass < 2; ++pass) {   // 0: the lane's output bytes; 1: behind the team's prefix sum, the stores
            int32_t st = r.start;
            uint32_t p = r.prev;
#pragma unroll
            for (uint32_t b = 0; b < 16u; ++b) {
                if (b < r.cnt) {
                    const uint32_t c = byte_of(r.v, b), pos = r.o + b, idx = mrle_index(c);
                    if (c != p) st = (int32_t)pos;
                    const uint32_t nx = b + 1u < r.cnt ? byte_of(r.v, (b + 1u) & 15u) : r.next;
                    if (!(idx < 6u && ((flags >> idx) & 1u))) {
                        if (pass && w < cap) dst[w] = (uint8_t)c;
                        w += 1u;
                    } else if (c != nx) {
                        const uint32_t L = pos - (uint32_t)st + 1u, full = (L - 1u) / 255u;
                        if (pass && w + 2u + full <= cap) {
                            dst[w] = (uint8_t)c;
                            for (uint32_t i = 0; i < full; ++i) dst[w + 1u + i] = 0xffu;
                            dst[w + 1u + full] = (uint8_t)(L - 255u * full - 1u);
                        }
                        w += 2u + full;
                    }
                    p = c;
                }
            }
            if (pass == 0) {
                uint32_t inc = w;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const uint32_t t = __shfl_up(inc, d, 16);
                    if (sub >= d) inc += t;
                }
                w = at + inc - w;   // where this lane's first output byte goes
                at += __shfl(inc, 15, 16);
            }
        }
    }
}

// off: the exclusive scan of psize; out: off[n] bytes
__global__ __launch_bounds__(kTxtThreads) void k_mrle_write(const uint8_t *__restrict__ text, const SortDesc *__restrict__ desc,
                                                            const uint64_t *__restrict__ off, const uint8_t *__restrict__ flag, uint32_t n,
                                                            uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, dst = 0;
        uint32_t qlen = 0, fl = 0, size = 0;
        if (k < n) {
            const SortDesc d = desc[k];
            src = d.off + d.qrel, qlen = d.qlen, dst = off[k], fl = flag[k];
            size = (uint32_t)(off[k + 1u] - dst) - 1u;
            out[dst] = (uint8_t)size, out[dst + 1u] = (uint8_t)fl;   // the size modulo 256, the flag byte
        }
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t fj = __shfl(fl, j, kWave);
            const uint32_t qj = __shfl(qlen, j, kWave), zj = __shfl(size, j, kWave);
            const uint32_t mj = k0 + (uint32_t)j < n ? qj : 0u;
            line_encode(text + sj, mj, wave_span(mj), fj, out + dj + 2u, zj - 1u, sub);
        }
    }
}

// the transitions of the decoder's two states (0: expects a symbol, 1: expects a count) as one map: bit s = the state behind state s
__device__ __forceinline__ uint32_t then(uint32_t first, uint32_t second) { return ((second >> (first & 1u)) & 1u) | (((second >> ((first >> 1) & 1u)) & 1u) << 1); }

// One record by 16 lanes: m token bytes at enc (behind the flag byte) -> len bytes at dst.  Uniform over the WAVE (ballots).
__device__ __forceinline__ void line_decode(const uint8_t *__restrict__ enc, uint32_t m, uint32_t steps, uint32_t flags, uint8_t *__restrict__ dst,
                                            uint32_t len, int sub, int grp)
{
    uint32_t state = 0, open = kNone, at = 0;   // carried over the steps: the state, the open token's symbol, decoded bytes so far
    for (uint32_t base = 0; base < steps; base += 256u) {
        u64 v[2];
        const uint32_t cnt = load_lane(enc, m, base + 16u * (uint32_t)sub, v);
        // 1. the lane's map, the team's scan of the maps: the state this lane starts in
        uint32_t s0 = 0, s1 = 1;
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b) {
            if (b < cnt) {
                const uint32_t c = byte_of(v, b), idx = mrle_index(c);
                const uint32_t sym = (idx < 6u && ((flags >> idx) & 1u)) ? 1u : 0u, more = c == 0xffu ? 1u : 0u;
                s0 = s0 ? more : sym, s1 = s1 ? more : sym;
            }
        }
        uint32_t inc = s0 | (s1 << 1);
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 16);
            if (sub >= d) inc = then(t, inc);
        }
        const uint32_t exm = __shfl_up(inc, 1, 16);
        const uint32_t entry = ((sub ? exm : 2u) >> state) & 1u;
        state = ((uint32_t)__shfl(inc, 15, 16) >> state) & 1u;
        // 2. decoded bytes of this lane, the last token symbol it saw: prefix sum, "last seen" scan
        uint32_t st = entry, produced = 0, seen = kNone;
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b) {
            if (b < cnt) {
                const uint32_t c = byte_of(v, b), idx = mrle_index(c);
                if (st == 0u) {
                    if (idx < 6u && ((flags >> idx) & 1u)) st = 1u, seen = c;
                    else produced += 1u;
                } else {
                    produced += c == 0xffu ? 255u : c + 1u;
                    if (c != 0xffu) st = 0u;
                }
            }
        }
        uint32_t pinc = produced, sinc = seen;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const uint32_t t = __shfl_up(pinc, d, 16), u = __shfl_up(sinc, d, 16);
            if (sub >= d) {
                pinc += t;
                if (sinc == kNone) sinc = u;
            }
        }
        uint32_t pos = at + pinc - produced;
        const uint32_t exs = __shfl_up(sinc, 1, 16);
        uint32_t sym = (sub && exs != kNone) ? exs : open;
        at += __shfl(pinc, 15, 16);
        const uint32_t last_seen = __shfl(sinc, 15, 16);
        if (last_seen != kNone) open = last_seen;
        // 3. the stores: a run of up to 8 bytes by its lane, a longer one by the team
        st = entry;
#pragma unroll 1
        for (uint32_t b = 0; b < 16u; ++b) {
            uint32_t run = 0, ch = 0, to = pos;
            if (b < cnt) {
                const uint32_t c = byte_of(v, b), idx = mrle_index(c);
                if (st == 0u) {
                    if (idx < 6u && ((flags >> idx) & 1u)) st = 1u, sym = c;
                    else run = 1u, ch = c;
                } else {
                    run = c == 0xffu ? 255u : c + 1u, ch = sym;
                    if (c != 0xffu) st = 0u;
                }
                pos += run;
                run = to >= len ? 0u : min(run, len - to);   // nothing behind the line's last byte, whatever the bytes say
            }
            if (run <= 8u)
                for (uint32_t i = 0; i < run; ++i) dst[to + i] = (uint8_t)ch;
            bool big = run > 8u;
            for (u64 any = __ballot(big); any; any = __ballot(big)) {
                const uint32_t mine = (uint32_t)(any >> (16 * grp)) & 0xffffu;
                if (mine) {
                    const int from = __builtin_ctz(mine);
                    const uint32_t t = __shfl(to, from, 16), rn = __shfl(run, from, 16), cc = __shfl(ch, from, 16);
                    for (uint32_t i = (uint32_t)sub; i < rn; i += 16u) dst[t + i] = (uint8_t)cc;
                    if (sub == from) big = false;
                }
            }
        }
    }
}

// poff / toff: the exclusive scans of psize / tsize; packed: what k_mrle_write wrote; out: toff[n] bytes
__global__ __launch_bounds__(kTxtThreads) void k_mrle_decode(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ poff,
                                                             const uint64_t *__restrict__ toff, uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t nwaves = gridDim.x * (kTxtThreads / kWave);
    const uint32_t wave = blockIdx.x * (kTxtThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    for (uint32_t k0 = wave * kWave; k0 < n; k0 += nwaves * kWave) {
        const uint32_t k = k0 + lane;
        u64 src = 0, dst = 0;
        uint32_t m = 0, len = 0, fl = 0;
        if (k < n) {
            src = poff[k] + 1u, dst = toff[k];
            m = (uint32_t)(poff[k + 1u] - src) - 1u, len = (uint32_t)(toff[k + 1u] - dst) - 1u;   // token bytes behind the flag byte; the line's length
            fl = packed[src];
            out[dst + len] = '\n';
        }
        for (int it = 0; it < kWave / 4; ++it) {
            if (k0 + 4u * (uint32_t)it >= n) break;
            const int j = 4 * it + grp;
            const u64 sj = __shfl(src, j, kWave), dj = __shfl(dst, j, kWave);
            const uint32_t fj = __shfl(fl, j, kWave), tj = __shfl(m, j, kWave), nj = __shfl(len, j, kWave);
            const bool live = k0 + (uint32_t)j < n;
            const uint32_t mj = live ? tj : 0u, lj = live ? nj : 0u;
            line_decode(packed + sj + 1u, mj, wave_span(mj), fj, out + dj, lj, sub, grp);
        }
    }
}

// the smallest r in [0, n) with off[r + 1] > edge (off ascending, off[n] > edge)
__device__ __forceinline__ uint32_t first_beyond(const uint64_t *__restrict__ off, uint32_t n, u64 edge)
{
    uint32_t lo = 0, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid + 1u] > edge) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// blocks of 4,096 bytes that have left a stream once its total is `total`: a buffer that is exactly full waits
__host__ __device__ __forceinline__ uint64_t blocks_left(uint64_t total) { return total ? (total - 1u) / kMrleBlock : 0u; }

// Workgroup B < nbt: text block B; B < nbt + nbp: packed block B - nbt; B == nbt + nbp: the packed remainder of `rest` bytes.
__global__ __launch_bounds__(256) void k_mrle_shared(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ poff,
                                                     const uint8_t *__restrict__ text, const uint64_t *__restrict__ toff, uint32_t n, u64 nbt, u64 nbp,
                                                     uint32_t rest, uint8_t *__restrict__ out)
{
    const u64 B = blockIdx.x;
    const uint8_t *src;
    u64 at;   // the block's place in the output, in blocks
    uint32_t bytes = kMrleBlock;
    if (B < nbt) {
        const uint32_t r = first_beyond(toff, n, (u64)kMrleBlock * (B + 1u));   // leaves during record r's text calls: ...
        at = B + blocks_left(poff[r]);                                          // ... behind the packed blocks that records < r pushed out
        src = text + (u64)kMrleBlock * B;
    } else if (B < nbt + nbp) {
        const u64 c = B - nbt;
        const uint32_t r = first_beyond(poff, n, (u64)kMrleBlock * (c + 1u));   // leaves during record r's packed calls: ...
        at = c + blocks_left(toff[r + 1u]);                                     // ... behind the text blocks that records <= r pushed out
        src = packed + (u64)kMrleBlock * c;
    } else {
        at = nbt + nbp, bytes = rest;
        src = packed + (u64)kMrleBlock * nbp;
    }
    if (at > nbt + nbp || (at == nbt + nbp) != (B == nbt + nbp)) return;   // (cannot be: every block has its own place in front of the remainder)
    uint8_t *dst = out + (u64)kMrleBlock * at;
    const uint32_t o = 16u * threadIdx.x;   // (both streams and the output start on 16-byte borders)
    if (o + 16u <= bytes) {
        u32 v;
        __builtin_memcpy(&v, src + o, 16);
        __builtin_memcpy(dst + o, &v, 16);
    } else {
        for (uint32_t b = o; b < bytes; ++b) dst[b] = src[b];
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

static inline unsigned team_blocks(uint32_t n, int n_cu)
{
    const uint64_t want = ((uint64_t)n + kTxtThreads - 1) / kTxtThreads, cap = (uint64_t)n_cu * 8;
    return (unsigned)(want < cap ? want : cap);
}

// d_bad: set to 0xffffffff here
hipError_t launch_mrle_sizes(const uint8_t *d_text, const void *d_desc, uint32_t n, uint32_t *d_psize, uint32_t *d_tsize, uint8_t *d_flag,
                             uint32_t *d_bad, int n_cu, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(k_mrle_sizes, dim3(team_blocks(n, n_cu)), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc, n, d_psize, d_tsize,
                       d_flag, d_bad);
    return hipGetLastError();
}

hipError_t launch_mrle_write(const uint8_t *d_text, const void *d_desc, const uint64_t *d_poff, const uint8_t *d_flag, uint32_t n,
                             uint8_t *d_packed, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mrle_write, dim3(team_blocks(n, n_cu)), dim3(kTxtThreads), 0, st, d_text, (const SortDesc *)d_desc, d_poff, d_flag, n,
                       d_packed);
    return hipGetLastError();
}

hipError_t launch_mrle_decode(const uint8_t *d_packed, const uint64_t *d_poff, const uint64_t *d_toff, uint32_t n, uint8_t *d_text_out, int n_cu,
                              hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mrle_decode, dim3(team_blocks(n, n_cu)), dim3(kTxtThreads), 0, st, d_packed, d_poff, d_toff, n, d_text_out);
    return hipGetLastError();
}

uint64_t mrle_shared_bytes(uint64_t packed_total, uint64_t text_total)
{
    const uint64_t nbp = blocks_left(packed_total);
    return kMrleBlock * (blocks_left(text_total) + nbp) + (packed_total - kMrleBlock * nbp);
}

// d_out holds mrle_shared_bytes(packed_total, text_total) bytes; n >= 1
hipError_t launch_mrle_shared(const uint8_t *d_packed, const uint64_t *d_poff, uint64_t packed_total, const uint8_t *d_text_out,
                              const uint64_t *d_toff, uint64_t text_total, uint32_t n, uint8_t *d_out, hipStream_t st)
{
    const uint64_t nbt = blocks_left(text_total), nbp = blocks_left(packed_total);
    if (nbt + nbp + 1u > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mrle_shared, dim3((unsigned)(nbt + nbp + 1u)), dim3(256), 0, st, d_packed, d_poff, d_text_out, d_toff, n, (u64)nbt, (u64)nbp,
                       (uint32_t)(packed_total - kMrleBlock * nbp), d_out);
    return hipGetLastError();
}

}  // namespace hpn
