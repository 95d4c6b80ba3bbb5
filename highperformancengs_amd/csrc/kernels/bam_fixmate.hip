// bam_fixmate.hip -- samtools' fixmate (bam_mate.c of samtools-0.1.19) on the device.  The reference is a state machine over the
// records in file order with one pending record; here it is closed forms over arrays.  (docs/kernels/bam_fixmate.md)
//
//   k_fix_classify   per record, in place through rec_off[] (hpn_bam_raw_index_dev): size 4 + block_size, where the record lies in
//                    the session's store, the class (refID < 0: skipped; flag 0x100: skipped; live), bam_calend by a one-lane walk
//                    over the CIGAR, flag 0x4 where the end lies beyond the target's length, the length of the CIGAR as text, and
//                    the domain checks (a CIGAR op above 8, a name with a NUL inside or none at its end, a refID the header lacks)
//   k_fix_live / k_fix_compact   the live records numbered by a scan and listed
//   k_fix_heads      16 lanes a live record: its name against the name of the live record in front of it, read from the store
//   k_fix_runstart   a scan of the heads numbers the runs of equal names; every run's first live ordinal
//   k_fix_roles      the position inside the run decides: odd closes a pair with the record in front, even opens one if the next
//                    live record has the same name, is a singleton otherwise, and the pending record if it is the last live one;
//                    and how many records the reference WRITES while record i is its current one (0, 1 or 2)
//   k_fix_plan       a scan of those counts gives every record's place in the output: order[]; and every record's patch -- flag,
//                    mate refID, mate pos, insert size, the CT field's length and the mate whose CIGAR it quotes
//   k_fix_apply      on a slice the gather has laid out with room behind every CT carrier: block_size and the four other core
//                    fields rewritten, "CTZ", both mates' CIGARs as text around the gap, a NUL.  Plain byte stores.
// No kernel waits for another workgroup.
#include "bam_fixmate.hpp"
#include "common.hpp"

namespace hpn {

namespace {

__device__ __forceinline__ uint32_t fx_word(const uint8_t *q)      // (records are not aligned: bytes)
{
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
}

__device__ __forceinline__ void fx_put(uint8_t *q, uint32_t v)
{
    q[0] = (uint8_t)v, q[1] = (uint8_t)(v >> 8), q[2] = (uint8_t)(v >> 16), q[3] = (uint8_t)(v >> 24);
}

__device__ __forceinline__ uint32_t fx_digits(uint32_t v)          // decimal digits of v (1 for 0)
{
    uint32_t d = 1;
    for (; v >= 10u; v /= 10u) ++d;
    return d;
}

__device__ __forceinline__ uint32_t fx_digits_signed(int32_t v)    // what kputw writes: a '-' in front of a negative number
{
    const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    return fx_digits(mag) + (v < 0 ? 1u : 0u);
}

__device__ __forceinline__ u64 fx_wave_min64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ u64 fx_wave_sum64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) v += __shfl_xor(v, d, kWave);
    return v;
}

// a writer that never leaves [w, lim): what does not fit is dropped (the lengths were computed from the same CIGARs)
struct FxText {
    uint8_t *w, *lim;
    __device__ __forceinline__ void put(uint8_t c)
    {
        if (w < lim) *w = c;
        ++w;
    }
    __device__ __forceinline__ void number(uint32_t mag)
    {
        uint8_t buf[10];
        int l = 0;
        do buf[l++] = (uint8_t)('0' + mag % 10u), mag /= 10u;
        while (mag);
        while (l) put(buf[--l]);
    }
};

// "1" or "2", "R" or "F", every op of the CIGAR as <len><chr> (ops 0..8: the domain)
__device__ __forceinline__ void fx_side(FxText &t, const uint8_t *rec, uint32_t flag)
{
    t.put(flag & 0x40u ? '1' : '2');
    t.put(flag & 0x10u ? 'R' : 'F');
    const uint32_t l_qname = rec[12], n_cigar = fx_word(rec + 16) & 0xffffu;
    const uint8_t *cg = rec + 36 + l_qname;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = fx_word(cg + 4 * (size_t)k);
        t.number(c >> 4);
        t.put((uint8_t)"MIDNSHP=X???????"[c & 15u]);
    }
}

__device__ __forceinline__ uint32_t fx_run_pos(uint32_t l, const uint32_t *head, const uint32_t *rid, const uint32_t *runstart)
{
    const uint32_t run = head[l] ? rid[l] : rid[l] - 1u;
    return l - runstart[run];
}

}  // namespace

__global__ __launch_bounds__(kFxThreads) void k_fix_classify(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                             uint64_t base, uint64_t store_at, uint32_t n_targets,
                                                             const uint32_t *__restrict__ target_len, uint32_t *__restrict__ size,
                                                             u64 *__restrict__ soff, uint32_t *__restrict__ meta, int32_t *__restrict__ cend,
                                                             uint32_t *__restrict__ clen, u64 *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    u64 bad = ~0ull;
    if (i < n) {
        const uint64_t first = rec_off[0], o = rec_off[i];
        const uint8_t *q = raw + o;
        const uint32_t bs = fx_word(q), tid = fx_word(q + 4), pos = fx_word(q + 8), l_qname = q[12], fn = fx_word(q + 16);
        const uint32_t n_cigar = fn & 0xffffu;
        uint32_t flag = fn >> 16, cls = kFxLive, end = pos, text = 0, reason = 0;
        if ((int32_t)tid < 0) {
            cls = kFxSkipTid;                  // written as it is: the reference looks at nothing else
        } else if (tid >= n_targets) {
            reason = kFxrTarget;
        } else if (bs < 32u || 32ull + l_qname + 4ull * n_cigar > bs) {
            reason = kFxrLayout;
        } else {
            const uint8_t *cg = q + 36 + l_qname;
            for (uint32_t k = 0; k < n_cigar; ++k) {
                const uint32_t c = fx_word(cg + 4 * (size_t)k), op = c & 15u, len = c >> 4;
                if (op > 8u) reason = kFxrCigarOp;
                if (0x3C1A7u >> (op << 1) & 2u) end += len;    // BAM_CIGAR_TYPE: the op consumes the reference
                text += fx_digits(len) + 1u;
            }
            if ((int32_t)end > (int32_t)target_len[tid]) flag |= 0x4u;
            if (flag & 0x100u) {
                cls = kFxSkipSecondary;
            } else if (!reason) {              // a live record's name is compared
                bool ok = l_qname != 0 && q[36 + l_qname - 1] == 0;
                for (uint32_t k = 0; k + 1 < l_qname; ++k) ok = ok && q[36 + k] != 0;
                if (!ok) reason = kFxrName;
            }
        }
        if (reason) bad = (base + i) << 3 | reason;
        size[base + i] = bs + 4u;
        soff[base + i] = store_at + (o - first);
        meta[base + i] = cls | flag << 16;
        cend[base + i] = (int32_t)end;
        clen[base + i] = text;
        if (i == 0) info[kBsFirst] = first;
        if (i == n - 1) info[kBsEnd] = o + 4 + (uint64_t)bs;
    }
    bad = fx_wave_min64(bad);
    if (lane_id() == 0 && bad != ~0ull) atomicMin(&info[kBsBad], bad);
}

__global__ __launch_bounds__(kFxThreads) void k_fix_live(const uint32_t *__restrict__ meta, uint64_t n, uint32_t *__restrict__ live)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (i < n) live[i] = (meta[i] & 3u) == kFxLive ? 1u : 0u;
}

__global__ __launch_bounds__(kFxThreads) void k_fix_compact(const uint32_t *__restrict__ meta, const uint32_t *__restrict__ lidx, uint64_t n,
                                                            uint32_t *__restrict__ liveidx)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (i < n && (meta[i] & 3u) == kFxLive) liveidx[lidx[i]] = (uint32_t)i;
}

// 16 lanes a live record.  In the domain a name's only NUL is its last byte, so strcmp is 0 exactly when the lengths and the
// bytes are equal.
__global__ __launch_bounds__(kFxThreads) void k_fix_heads(FxRecords r, const uint32_t *__restrict__ liveidx, uint64_t n_live,
                                                          uint32_t *__restrict__ head)
{
    const uint64_t l = ((uint64_t)blockIdx.x * kFxThreads + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    uint32_t differ = 0;
    if (l < n_live) {
        if (l == 0) {
            differ = 1;
        } else {
            const uint8_t *a = r.store + r.soff[liveidx[l]], *b = r.store + r.soff[liveidx[l - 1]];
            const uint32_t la = a[12], lb = b[12];
            if (la != lb) differ = 1;
            else
                for (uint32_t k = sub; k < la; k += 16u) differ |= a[36 + k] != b[36 + k] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int d = 1; d < 16; d *= 2) differ |= __shfl_xor(differ, d, kWave);
    if (l < n_live && sub == 0) head[l] = differ;
}

__global__ __launch_bounds__(kFxThreads) void k_fix_runstart(const uint32_t *__restrict__ head, const uint32_t *__restrict__ rid, uint64_t n_live,
                                                             uint32_t *__restrict__ runstart)
{
    const uint64_t l = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (l < n_live && head[l]) runstart[rid[l]] = (uint32_t)l;
}

__global__ __launch_bounds__(kFxThreads) void k_fix_roles(const uint32_t *__restrict__ meta, const uint32_t *__restrict__ lidx, uint64_t n,
                                                          uint64_t n_live, const uint32_t *__restrict__ head, const uint32_t *__restrict__ rid,
                                                          const uint32_t *__restrict__ runstart, int remove_reads, uint32_t *__restrict__ role,
                                                          uint32_t *__restrict__ writes)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (i >= n) return;
    if ((meta[i] & 3u) != kFxLive) {
        role[i] = kFxSkipped, writes[i] = remove_reads ? 0u : 1u;
        return;
    }
    const uint32_t l = lidx[i], at = fx_run_pos(l, head, rid, runstart);
    const bool next_same = (uint64_t)l + 1 < n_live && !head[l + 1];
    // a record is pending when l arrives exactly when the live record in front of l stands at an even place of its run
    const bool pending = l > 0 && (fx_run_pos(l - 1, head, rid, runstart) & 1u) == 0;
    role[i] = at & 1u ? kFxSecond : next_same ? kFxFirst : (uint64_t)l + 1 == n_live ? kFxPending : kFxSingle;
    writes[i] = (pending ? 1u : 0u) + (at & 1u);
}

__global__ __launch_bounds__(kFxThreads) void k_fix_plan(FxRecords r, const uint32_t *__restrict__ lidx, const uint32_t *__restrict__ liveidx,
                                                         uint64_t n, const uint32_t *__restrict__ role, const uint32_t *__restrict__ writes,
                                                         const uint32_t *__restrict__ woff, uint32_t *__restrict__ order, FxPatch p,
                                                         u64 *__restrict__ info)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    u64 pairs = 0, singles = 0, tags = 0, added = 0;
    if (i < n) {
        const uint8_t *q = r.store + r.soff[i];
        const uint32_t ro = role[i];
        uint32_t flag = r.meta[i] >> 16, mtid = fx_word(q + 24), mpos = fx_word(q + 28), isize = fx_word(q + 32), extra = 0, mate = (uint32_t)i;
        uint32_t slot = ~0u;
        if (ro == kFxSkipped) {
            if (writes[i]) slot = woff[i];
        } else if (ro == kFxPending) {
            slot = woff[n];                    // behind everything a record triggered: written as it is
        } else if (ro == kFxSingle) {
            slot = woff[liveidx[lidx[i] + 1]]; // the next live record writes it first
            mtid = mpos = ~0u, isize = 0;
            if (flag & 0x1u) flag = (flag | 0x8u) & ~(0x20u | 0x2u);
            singles = 1;
        } else {
            const bool am_first = ro == kFxFirst;
            const uint32_t j = am_first ? liveidx[lidx[i] + 1] : liveidx[lidx[i] - 1];
            const uint8_t *o = r.store + r.soff[j];
            const uint32_t tid = fx_word(q + 4), pos = fx_word(q + 8), otid = fx_word(o + 4), opos = fx_word(o + 8), oflag = r.meta[j] >> 16;
            const uint32_t end = (uint32_t)r.cend[i], oend = (uint32_t)r.cend[j];
            slot = am_first ? woff[j] : woff[i] + 1u;
            mate = j, mtid = otid, mpos = opos;
            if (tid == otid && !(flag & 0xcu) && !(oflag & 0xcu)) isize = (oflag & 0x10u ? oend : opos) - (flag & 0x10u ? end : pos);   // (uint32_t, as the reference)
            else isize = 0;
            flag = oflag & 0x10u ? flag | 0x20u : flag & ~0x20u;
            if (oflag & 0x4u) flag = (flag | 0x8u) & ~0x2u;
            if (tid == otid) {
                // bam_template_cigar(pre, cur): the record with the smaller pos carries the tag, the earlier one on a tie
                const int32_t fpos = (int32_t)(am_first ? pos : opos), spos = (int32_t)(am_first ? opos : pos);
                const bool first_carries = !(fpos > spos);
                if (first_carries == am_first) {
                    const int32_t gap = (int32_t)(opos - end);
                    const uint32_t text = 2u + r.clen[i] + fx_digits_signed(gap) + 1u + 2u + r.clen[j];
                    extra = 4u + text, tags = 1, added = extra;
                }
            }
            if (am_first) pairs = 1;
        }
        if (slot != ~0u) order[slot] = (uint32_t)i;
        p.flag[i] = flag, p.mtid[i] = mtid, p.mpos[i] = mpos, p.isize[i] = isize, p.extra[i] = extra, p.partner[i] = mate;
    }
    pairs = fx_wave_sum64(pairs), singles = fx_wave_sum64(singles), tags = fx_wave_sum64(tags), added = fx_wave_sum64(added);
    if (lane_id() == 0) {
        if (pairs) atomicAdd(&info[kFxPairs], pairs);
        if (singles) atomicAdd(&info[kFxSingles], singles);
        if (tags) atomicAdd(&info[kFxTags], tags);
        if (added) atomicAdd(&info[kFxAdded], added);
    }
}

__global__ __launch_bounds__(kFxThreads) void k_fix_apply(FxRecords r, FxPatch p, const uint32_t *__restrict__ order,
                                                          const u64 *__restrict__ out_off, uint64_t first, uint64_t cnt, uint8_t *__restrict__ pay)
{
    const uint64_t k = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t i = order[first + k], len = r.size[i], extra = p.extra[i], flag = p.flag[i];
    uint8_t *d = pay + (out_off[first + k] - out_off[first]);
    fx_put(d, len - 4u + extra);
    d[18] = (uint8_t)flag, d[19] = (uint8_t)(flag >> 8);
    fx_put(d + 24, p.mtid[i]), fx_put(d + 28, p.mpos[i]), fx_put(d + 32, p.isize[i]);
    if (!extra) return;
    const uint32_t j = p.partner[i];
    const uint8_t *lower = r.store + r.soff[i], *upper = r.store + r.soff[j];
    FxText t = {d + len, d + len + extra};
    t.put('C'), t.put('T'), t.put('Z');
    fx_side(t, lower, flag);
    const int32_t gap = (int32_t)(fx_word(upper + 8) - (uint32_t)r.cend[i]);
    if (gap < 0) t.put('-');
    t.number(gap < 0 ? 0u - (uint32_t)gap : (uint32_t)gap);
    t.put('T');
    fx_side(t, upper, p.flag[j]);
    t.put(0);
}

static inline unsigned fx_grid(uint64_t n) { return (unsigned)((n + kFxThreads - 1) / kFxThreads); }

hipError_t launch_bamfix_classify(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, uint32_t n_targets,
                                  const uint32_t *target_len, uint32_t *size, u64 *soff, uint32_t *meta, int32_t *cend, uint32_t *clen, u64 *info,
                                  hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fix_classify, dim3(fx_grid(n)), dim3(kFxThreads), 0, st, raw, rec_off, n, base, store_at, n_targets, target_len, size, soff, meta,
                       cend, clen, info);
    return hipGetLastError();
}

hipError_t launch_bamfix_live(const uint32_t *meta, uint64_t n, uint32_t *live, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fix_live, dim3(fx_grid(n)), dim3(kFxThreads), 0, st, meta, n, live);
    return hipGetLastError();
}

hipError_t launch_bamfix_compact(const uint32_t *meta, const uint32_t *lidx, uint64_t n, uint32_t *liveidx, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fix_compact, dim3(fx_grid(n)), dim3(kFxThreads), 0, st, meta, lidx, n, liveidx);
    return hipGetLastError();
}

hipError_t launch_bamfix_heads(FxRecords r, const uint32_t *liveidx, uint64_t n_live, uint32_t *head, hipStream_t st)
{
    if (!n_live) return hipSuccess;
    hipLaunchKernelGGL(k_fix_heads, dim3(fx_grid(n_live * 16)), dim3(kFxThreads), 0, st, r, liveidx, n_live, head);
    return hipGetLastError();
}

hipError_t launch_bamfix_runstart(const uint32_t *head, const uint32_t *rid, uint64_t n_live, uint32_t *runstart, hipStream_t st)
{
    if (!n_live) return hipSuccess;
    hipLaunchKernelGGL(k_fix_runstart, dim3(fx_grid(n_live)), dim3(kFxThreads), 0, st, head, rid, n_live, runstart);
    return hipGetLastError();
}

hipError_t launch_bamfix_roles(const uint32_t *meta, const uint32_t *lidx, uint64_t n, uint64_t n_live, const uint32_t *head, const uint32_t *rid,
                               const uint32_t *runstart, int remove_reads, uint32_t *role, uint32_t *writes, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fix_roles, dim3(fx_grid(n)), dim3(kFxThreads), 0, st, meta, lidx, n, n_live, head, rid, runstart, remove_reads, role, writes);
    return hipGetLastError();
}

hipError_t launch_bamfix_plan(FxRecords r, const uint32_t *lidx, const uint32_t *liveidx, uint64_t n, const uint32_t *role, const uint32_t *writes,
                              const uint32_t *woff, uint32_t *order, FxPatch p, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fix_plan, dim3(fx_grid(n)), dim3(kFxThreads), 0, st, r, lidx, liveidx, n, role, writes, woff, order, p, info);
    return hipGetLastError();
}

hipError_t launch_bamfix_apply(FxRecords r, FxPatch p, const uint32_t *order, const u64 *out_off, uint64_t first, uint64_t cnt, uint8_t *pay,
                               hipStream_t st)
{
    if (!cnt) return hipSuccess;
    hipLaunchKernelGGL(k_fix_apply, dim3(fx_grid(cnt)), dim3(kFxThreads), 0, st, r, p, order, out_off, first, cnt, pay);
    return hipGetLastError();
}

}  // namespace hpn
