// bam_rmdup.hip -- samtools' rmdup of a coordinate-sorted BAM (bam_rmdup.c: bam_rmdup_core) on the device: which records survive
// and where they go.  The reference decides record by record with a hash of groups, a stack and a set of names; here the same
// decisions come from the records' left neighbours, a stable sort of the heads, a walk over each group, a stable sort of the name
// events and two scans.  (docs/kernels/bam_rmdup.md has the rules and the derivation.)
//
//   k_rm_classify   per record, in place through rec_off[] (hpn_bam_raw_index_dev): the fixed fields, the class (written at once /
//                   head / tail / unplaced), the domain checks against the left neighbour; then 16 lanes a record: the name's
//                   hash and its NUL check for heads and tails, the sum of the quality bytes for heads; one lane of the team
//                   walks a head's aux fields to its RG and looks the value up in the header's ID table
//   k_rm_runs       run boundaries ((refID, pos) differs from the left neighbour) and head flags, the events' first state
//   k_rm_scatter    run ordinals, every run's first record, the heads compacted with their key (library << 32 | isize)
//   k_rm_runkey     the heads' second key: the run ordinal (the radix sort is stable: two passes give (run, library, isize))
//   k_rm_groups     one lane a group: the slot (the group's first record), the survivor (the first record that attains the largest
//                   sum), every loser's insertion into the name set at the time the reference makes it; counts per library
//   k_rm_evkey      the events in time order -> (name hash, time) for the sort
//   k_rm_names      the left-neighbour rule over the sorted events: dropped tails, inconsistent insertions, unmatched names; equal
//                   hashes are verified byte for byte
//   k_rm_flags      written-at-once and slot flags for the two scans
//   k_rm_place      every survivor's output index: order[]
#include "common.hpp"
#include "bam_rmdup.hpp"

namespace hpn {

constexpr int kRmThreads = 256;

__device__ __forceinline__ uint32_t rm_word(const uint8_t *q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; }

__device__ __forceinline__ u64 team_sum64(u64 v)      // over the 16 lanes of a team
{
#pragma unroll
    for (int d = 1; d < 16; d *= 2) v += __shfl_xor(v, d, kWave);
    return v;
}
__device__ __forceinline__ uint32_t team_sum32(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < 16; d *= 2) v += __shfl_xor(v, d, kWave);
    return v;
}
__device__ __forceinline__ u64 wave_min_u64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

// bam_aux_get(b, "RG") for a head whose aux fields lie in [s, e): the library of its RG value (0: no RG, or an ID the table does
// not have), or a reason in *reason.  Only the types of the format are walked; bam_aux_get's own reading of anything else
// (it upper-cases the type and gives what it does not know no size) is the host's.
__device__ uint32_t rm_library(const uint8_t *__restrict__ r, uint32_t s, uint32_t e, const RmIds &ids, uint32_t *reason)
{
    while (s < e) {
        if (s + 3 > e) return *reason = kRsAux, 0u;
        const bool is_rg = r[s] == 'R' && r[s + 1] == 'G';
        const uint8_t ty = r[s + 2];
        s += 3;
        if (is_rg && ty != 'Z') return *reason = kRsRgType, 0u;
        uint32_t step = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': step = 1; break;
        case 's': case 'S': step = 2; break;
        case 'i': case 'I': case 'f': step = 4; break;
        case 'Z': case 'H': {
            const uint32_t from = s;
            while (s < e && r[s]) ++s;
            if (s >= e) return *reason = kRsAux, 0u;
            if (is_rg) {
                const uint32_t len = s - from;
                for (uint32_t k = 0; k < ids.n; ++k) {
                    const uint32_t a = ids.off[k];
                    if (ids.off[k + 1] - a != len) continue;
                    uint32_t i = 0;
                    while (i < len && ids.bytes[a + i] == r[from + i]) ++i;
                    if (i == len) return ids.lib[k];
                }
                return 0u;
            }
            ++s;
            continue;
        }
        case 'B': {
            if (s + 5 > e) return *reason = kRsAux, 0u;
            const uint8_t sub = r[s];
            const uint32_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            const int32_t cnt = (int32_t)rm_word(r + s + 1);
            if (!w || cnt < 0 || (u64)s + 5 + (u64)w * (u64)cnt > e) return *reason = kRsAux, 0u;
            s += 5 + w * (uint32_t)cnt;
            continue;
        }
        default: return *reason = kRsAux, 0u;
        }
        s += step;
        if (s > e) return *reason = kRsAux, 0u;
    }
    return 0u;
}

__global__ __launch_bounds__(kRmThreads) void k_rm_classify(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t base,
                                                            uint64_t store_at, uint32_t n_ref, RmArrays A, RmIds ids, u64 *__restrict__ info)
{
    const uint64_t wave = (uint64_t)blockIdx.x * (kRmThreads / kWave) + wave_id();
    const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
    const uint64_t k0 = wave * kWave, i = k0 + lane;
    if (k0 >= n) return;
    // one lane a record: fields, class, the checks against the left neighbour
    u64 at = 0;
    uint32_t size = 0, cls = kRmPass, reason = 0, l_qname = 0, n_cigar = 0, tid = 0;
    int32_t l_qseq = 0;
    if (i < n) {
        const uint64_t first = rec_off[0];
        at = rec_off[i];
        const uint8_t *q = raw + at;
        size = rm_word(q) + 4u;
        tid = rm_word(q + 4);
        const int32_t pos = (int32_t)rm_word(q + 8), mtid = (int32_t)rm_word(q + 24), isz = (int32_t)rm_word(q + 32);
        const uint32_t flag = rm_word(q + 16) >> 16;
        l_qname = q[12], n_cigar = rm_word(q + 16) & 0xffffu, l_qseq = (int32_t)rm_word(q + 20);
        const uint64_t g = base + i;
        u64 left = ~0ull;          // the left neighbour's (refID, pos) word; ~0: it is unplaced
        bool has_left = g != 0;
        if (i) {
            const uint8_t *p = raw + rec_off[i - 1];
            const uint32_t lt = rm_word(p + 4);
            left = lt == 0xffffffffu ? ~0ull : (u64)lt << 32 | rm_word(p + 8);
        } else if (has_left) {
            const u64 w = A.tp[g - 1];
            left = (w >> 32) == 0xffffffffull ? ~0ull : w;
        }
        if (tid == 0xffffffffu) {
            cls = kRmUnplaced;
            if (!has_left) reason = kRsFirstUnplaced;
        } else {
            if (has_left && (left == ~0ull || tid < (uint32_t)(left >> 32))) reason = kRsTidBack;
            else if (tid >= n_ref) reason = kRsTidBeyond;
            else if (pos < 0) reason = kRsPosNeg;
            else if (has_left && tid == (uint32_t)(left >> 32) && (uint32_t)pos < (uint32_t)left) reason = kRsPosBack;
            if (!(flag & 1u) || (flag & 12u) || (mtid >= 0 && (uint32_t)mtid != tid)) cls = kRmPass;
            else cls = isz > 0 ? kRmHead : kRmTail;
        }
        A.tp[g] = cls == kRmUnplaced ? 0xffffffffull << 32 : (u64)tid << 32 | (uint32_t)pos;
        A.cls[g] = cls, A.isize[g] = (uint32_t)isz, A.size[g] = size, A.soff[g] = store_at + (at - first);
        A.qsum[g] = 0, A.lib[g] = 0, A.hash[g] = 0;
        if (i == 0) info[kRmFirst] = first;
        if (i == n - 1) info[kRmEnd] = at + size;
    }
    // 16 lanes a record: the names of heads and tails, the qualities and the library of heads
    const bool want = i < n && !reason && (cls == kRmHead || cls == kRmTail);
    for (int it = 0; it < kWave / 4; ++it) {
        if (k0 + 4u * (uint64_t)it >= n) break;
        const int j = 4 * it + grp;
        const u64 aj = __shfl(at, j, kWave);
        const uint32_t sj = __shfl(size, j, kWave), cj = __shfl(cls, j, kWave), lqn = __shfl(l_qname, j, kWave), ncg = __shfl(n_cigar, j, kWave),
                       tj = __shfl(tid, j, kWave);
        const int32_t lqs = __shfl(l_qseq, j, kWave);
        const bool wj = __shfl((int)want, j, kWave) != 0;
        if (!wj) continue;              // (the same for all 16 lanes of the team)
        const uint8_t *r = raw + aj;
        uint32_t rj = 0;
        u64 h = 0;
        if (lqn == 0 || 36u + lqn > sj) {
            rj = kRsName;
        } else {
            uint32_t nul = 0;
            for (uint32_t k = (uint32_t)sub; k + 1 < lqn; k += 16) {
                const uint8_t c = r[36 + k];
                nul |= c == 0;
                h += mix64(kGold * (u64)(k + 1) ^ (u64)c << 32 ^ c);
            }
            if (sub == 0 && r[36 + lqn - 1] != 0) nul = 1;
            nul = team_sum32(nul);
            h = team_sum64(h);
            if (nul) rj = kRsName;
            h = mix64(h + kStep * (u64)lqn + ((u64)tj << 32 | tj));
            if (h == ~0ull) h = ~0ull - 1;          // (~0 marks "no event" in the sort)
        }
        uint32_t qsum = 0, lib = 0;
        if (!rj && cj == kRmHead) {
            const u64 q0 = 36ull + lqn + 4ull * ncg + (u64)(((int64_t)lqs + 1) / 2);
            if (lqs < 0 || q0 + (u64)lqs > sj) {
                rj = kRsFields;
            } else {
                for (uint32_t k = (uint32_t)sub; k < (uint32_t)lqs; k += 16) qsum += r[q0 + k];
                qsum = team_sum32(qsum);
                uint32_t ra = 0;
                if (sub == 0) lib = rm_library(r, (uint32_t)(q0 + (u64)lqs), sj, ids, &ra);
                rj = __shfl(ra, lane & ~15, kWave);
            }
        }
        if (sub == 0) {
            const uint64_t g = base + k0 + (uint64_t)j;
            A.hash[g] = h, A.qsum[g] = qsum, A.lib[g] = lib;
            if (rj) atomicMin(&info[kRmBad], g << 4 | rj);      // (rare: a team's own word)
        }
    }
    u64 bad = reason && i < n ? (base + i) << 4 | reason : ~0ull;
    bad = wave_min_u64(bad);
    if (lane == 0 && bad != ~0ull) atomicMin(&info[kRmBad], bad);
}

// present: n_ref + 1 flags -- target t has records; [n_ref]: unplaced records follow the placed ones
__global__ __launch_bounds__(kRmThreads) void k_rm_runs(RmArrays A, RmWork W, uint64_t n, uint32_t n_ref, uint32_t *__restrict__ present)
{
    const uint64_t i = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t cls = A.cls[i];
    W.rb[i] = i == 0 || A.tp[i] != A.tp[i - 1];
    if (i == 0 || (A.tp[i] >> 32) != (A.tp[i - 1] >> 32)) {
        const u64 tid = A.tp[i] >> 32;
        present[tid < n_ref ? tid : n_ref] = 1u;
    }
    W.hf[i] = cls == kRmHead;
    W.evkind[i] = cls == kRmTail ? kEvTail : kEvNone;
    W.evrec[i] = (uint32_t)i;
    W.slot[i] = 0, W.drop[i] = 0;
}

__global__ __launch_bounds__(kRmThreads) void k_rm_scatter(RmArrays A, RmWork W, uint64_t n, u64 *__restrict__ hkey, uint32_t *__restrict__ hval)
{
    const uint64_t i = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t rid = W.rsc[i] + W.rb[i] - 1u;
    W.rid[i] = rid;
    if (W.rb[i]) W.runstart[rid] = (uint32_t)i;
    if (i == n - 1) W.runstart[W.rsc[n]] = (uint32_t)n;
    if (W.hf[i]) {
        const uint32_t k = W.hsc[i];
        hkey[k] = (u64)A.lib[i] << 32 | A.isize[i];
        hval[k] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kRmThreads) void k_rm_runkey(RmWork W, uint64_t m, u64 *__restrict__ hkey, const uint32_t *__restrict__ hval)
{
    const uint64_t k = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (k < m) hkey[k] = W.rid[hval[k]];
}

__device__ __forceinline__ bool rm_same_group(const RmArrays &A, const RmWork &W, uint32_t a, uint32_t b)
{
    return W.rid[a] == W.rid[b] && A.lib[a] == A.lib[b] && A.isize[a] == A.isize[b];
}

// libs: three words a library -- heads, heads removed, the first head's ordinal (~0 none)
__global__ __launch_bounds__(kRmThreads) void k_rm_groups(RmArrays A, RmWork W, uint64_t m, const uint32_t *__restrict__ hval, u64 *__restrict__ libs)
{
    const uint64_t j = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (j >= m) return;
    const uint32_t first = hval[j];
    if (j && rm_same_group(A, W, first, hval[j - 1])) return;      // (only a group's first head walks it)
    uint32_t holder = first, best = A.qsum[first];
    uint64_t e = j + 1;
    for (; e < m; ++e) {
        const uint32_t b = hval[e];
        if (!rm_same_group(A, W, first, b)) break;
        const uint32_t s = A.qsum[b];
        if ((int32_t)best < (int32_t)s) {          // sum_qual is an int
            W.evrec[b] = holder;                   // the holder's name goes into the set while b is being read
            holder = b, best = s;
        } else {
            W.evrec[b] = b;
        }
        W.evkind[b] = kEvIns;
    }
    W.slot[first] = holder + 1u;
    u64 *l = libs + 3 * (size_t)A.lib[first];
    atomicAdd(&l[0], (u64)(e - j));
    atomicAdd(&l[1], (u64)(e - j - 1));
    atomicMin(&l[2], (u64)first);
}

__global__ __launch_bounds__(kRmThreads) void k_rm_evkey(RmArrays A, RmWork W, uint64_t n, u64 *__restrict__ ekey, uint32_t *__restrict__ eval)
{
    const uint64_t i = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    ekey[i] = W.evkind[i] == kEvNone ? ~0ull : A.hash[W.evrec[i]];
    eval[i] = (uint32_t)i;
}

// the names of records a and b (both heads or tails whose names have been checked) as they lie in the store
__device__ bool rm_same_name(const uint8_t *__restrict__ store, const RmArrays &A, uint32_t a, uint32_t b)
{
    const uint8_t *p = store + A.soff[a], *q = store + A.soff[b];
    const uint32_t len = p[12];
    if (len != q[12] || (A.tp[a] >> 32) != (A.tp[b] >> 32)) return false;
    for (uint32_t k = 0; k < len; ++k)
        if (p[36 + k] != q[36 + k]) return false;
    return true;
}

__global__ __launch_bounds__(kRmThreads) void k_rm_names(const uint8_t *__restrict__ store, RmArrays A, RmWork W, uint64_t n, const u64 *__restrict__ ekey,
                                                         const uint32_t *__restrict__ eval, u64 *__restrict__ unmatched, u64 *__restrict__ info)
{
    const uint64_t j = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t t = eval[j], kind = W.evkind[t];
    if (kind == kEvNone) return;
    const u64 h = ekey[j];
    const uint32_t x = W.evrec[t];
    uint32_t left = kEvNone;
    if (j && ekey[j - 1] == h) {
        const uint32_t tl = eval[j - 1];
        left = W.evkind[tl];
        if (left != kEvNone && !rm_same_name(store, A, x, W.evrec[tl])) {
            atomicMin(&info[kRmBad], (u64)t << 4 | kRsCollision);
            return;
        }
    }
    if (kind == kEvTail) {
        if (left == kEvIns) W.drop[t] = 1;
        return;
    }
    if (left == kEvIns) atomicMin(&info[kRmBad], (u64)t << 4 | kRsInconsistent);
    const bool more = j + 1 < n && ekey[j + 1] == h && W.evkind[eval[j + 1]] != kEvNone;
    if (!more) atomicAdd(&unmatched[A.tp[x] >> 32], 1ull);      // the name's last event is an insertion
}

__global__ __launch_bounds__(kRmThreads) void k_rm_flags(RmArrays A, RmWork W, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t cls = A.cls[i];
    W.now[i] = cls == kRmPass || cls == kRmUnplaced || (cls == kRmTail && !W.drop[i]);
    W.sl[i] = W.slot[i] != 0;
}

// Inside a run everything written at once comes first, in file order, then the slots in the order their groups began:
//   written at once:  (such records in front of i) + (slots in front of i's run)
//   a slot:           (such records up to the end of i's run) + (slots in front of i)
__global__ __launch_bounds__(kRmThreads) void k_rm_place(RmWork W, uint64_t n, uint64_t n_out, uint32_t *__restrict__ order)
{
    const uint64_t i = (uint64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t rid = W.rid[i];
    if (W.now[i]) {
        const uint64_t at = (uint64_t)W.cnow[i] + W.cslot[W.runstart[rid]];
        if (at < n_out) order[at] = (uint32_t)i;
    }
    if (W.sl[i]) {
        const uint64_t at = (uint64_t)W.cnow[W.runstart[rid + 1]] + W.cslot[i];
        if (at < n_out) order[at] = W.slot[i] - 1u;
    }
}

static inline unsigned rm_grid(uint64_t n) { return (unsigned)((n + kRmThreads - 1) / kRmThreads); }

hipError_t launch_rmdup_classify(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, uint32_t n_ref, const RmArrays &A,
                                 const RmIds &ids, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_classify, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, raw, rec_off, n, base, store_at, n_ref, A, ids, info);
    return hipGetLastError();
}

hipError_t launch_rmdup_runs(const RmArrays &A, const RmWork &W, uint64_t n, uint32_t n_ref, uint32_t *present, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_runs, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, A, W, n, n_ref, present);
    return hipGetLastError();
}

hipError_t launch_rmdup_scatter(const RmArrays &A, const RmWork &W, uint64_t n, u64 *hkey, uint32_t *hval, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_scatter, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, A, W, n, hkey, hval);
    return hipGetLastError();
}

hipError_t launch_rmdup_runkey(const RmWork &W, uint64_t m, u64 *hkey, const uint32_t *hval, hipStream_t st)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_rm_runkey, dim3(rm_grid(m)), dim3(kRmThreads), 0, st, W, m, hkey, hval);
    return hipGetLastError();
}

hipError_t launch_rmdup_groups(const RmArrays &A, const RmWork &W, uint64_t m, const uint32_t *hval, u64 *libs, hipStream_t st)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_rm_groups, dim3(rm_grid(m)), dim3(kRmThreads), 0, st, A, W, m, hval, libs);
    return hipGetLastError();
}

hipError_t launch_rmdup_evkey(const RmArrays &A, const RmWork &W, uint64_t n, u64 *ekey, uint32_t *eval, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_evkey, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, A, W, n, ekey, eval);
    return hipGetLastError();
}

hipError_t launch_rmdup_names(const uint8_t *store, const RmArrays &A, const RmWork &W, uint64_t n, const u64 *ekey, const uint32_t *eval, u64 *unmatched,
                              u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_names, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, store, A, W, n, ekey, eval, unmatched, info);
    return hipGetLastError();
}

hipError_t launch_rmdup_flags(const RmArrays &A, const RmWork &W, uint64_t n, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_flags, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, A, W, n);
    return hipGetLastError();
}

hipError_t launch_rmdup_place(const RmWork &W, uint64_t n, uint64_t n_out, uint32_t *order, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rm_place, dim3(rm_grid(n)), dim3(kRmThreads), 0, st, W, n, n_out, order);
    return hipGetLastError();
}

}  // namespace hpn
