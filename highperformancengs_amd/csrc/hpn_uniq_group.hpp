// hpn_uniq_group.hpp -- the grouping stage that hpn_fastq_uniq_* (hpn_uniq.hip), hpn_fastq_uniqq_* (hpn_uniqq.hip) and
// hpn_fastq_usort_* (hpn_usort.hip) share: the session (hpn_store.hpp) with the stage's arrays, uniq_match_mates() -- the name
// check of a paired session -- and uniq_group(): pair keys, the stable sort by grouping hash, flags, the host's ordering of clashing runs,
// group scan, reduce, the table-walk key and the sdscmp order.  Kernels: kernels/fastq_uniq.hip, kernels/radix_sort.hpp.
//
// dict.c's walk in closed form (derived from its rehashing: a table of 4 that doubles when full; a doubling walks the old
// chains head to tail and pushes onto the new heads, so it reverses them; new keys go to the head).  With h = djb2 of the
// key, j = the key's rank by first occurrence, e(j) = 0 for j < 4 else floor(log2 j) - 1, U keys:
//   S = smallest power of two >= max(U, 4), K = e(U - 1);
//   if U is a power of two >= 4 and a record behind the last first occurrence replaced its key's representative, the
//   full table doubled once more inside dictReplace's dictAdd: S = 2 U, K = e(U - 1) + 1 (a caller that never calls
//   dictReplace -- gzfastq_uniqQ.c -- passes replace_doubles = false);
//   the keys come in ascending (h & (S - 1), p, p ? j : -j), p = (K - e(j)) & 1.
#pragma once
#include <string.h>

#include <algorithm>
#include <string>

#include "hpn_store.hpp"

namespace hpn {
// kernels/fastq_uniq.hip
hipError_t launch_uniq_keys(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                            void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *user);
hipError_t launch_uniqq_keys(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                             void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *user);
hipError_t launch_uniq_names(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, uint32_t n, uint32_t *d_first_bad,
                             hipStream_t st);
hipError_t launch_uniq_pair(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, uint32_t n,
                            uint64_t hash_mask, uint64_t *d_hash, uint32_t *d_order, uint32_t *d_djb, uint32_t *d_sumq, uint32_t *d_info,
                            hipStream_t st);
hipError_t launch_uniq_flags(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint64_t *d_hash,
                             const uint32_t *d_order, uint32_t n, uint32_t *d_flag, uint32_t *d_info, hipStream_t st);
hipError_t launch_uniq_reduce(const uint32_t *d_order, const uint32_t *d_flag, const uint32_t *d_gid, const uint32_t *d_sumq, uint32_t n,
                              uint32_t n_groups, uint32_t *d_count, uint64_t *d_best, uint32_t *d_first, uint32_t *d_rep, uint32_t *d_info,
                              hipStream_t st);
hipError_t launch_uniq_mark(const uint32_t *d_first, uint32_t n_groups, uint32_t *d_mark, uint32_t n, hipStream_t st);
hipError_t launch_uniq_table_key(const uint32_t *d_first, const uint32_t *d_rank, const uint32_t *d_djb, uint32_t n_groups,
                                 uint32_t size_mask, uint32_t K, uint64_t *d_key, uint32_t *d_val, hipStream_t st);
hipError_t launch_uniq_iota(uint32_t n, uint32_t *d_val, hipStream_t st);
hipError_t launch_uniq_seq_word(const uint8_t *t0, const void *d0, const uint32_t *d_first, const uint32_t *d_val, uint32_t n_groups,
                                uint32_t w, uint64_t *d_key, hipStream_t st);
hipError_t launch_uniq_sizes(const void *d_desc, const uint32_t *d_list, const uint32_t *d_rep, const uint32_t *d_count, uint32_t n_groups,
                             uint32_t *d_size, hipStream_t st);
hipError_t launch_uniq_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_list, const uint32_t *d_rep,
                             const uint32_t *d_count, const uint64_t *d_off, uint32_t n_groups, uint8_t *d_out, int n_cu, hipStream_t st);

// The family's words of the session's info block.  The kernels of fastq_uniq.hip (words 0 .. 3) and fastq_usort.hip (7 .. 11)
// number them from kUiBase on: they are handed uniq_kinfo().
enum { kUiBase = kInfoOwn, kUiMaxLen = kUiBase, kUiClash, kUiLastFirst, kUiBehind, kUiFirstBad, kUiMaxCount };
constexpr size_t kUniqDescBytes = 32;     // kernels/uniq_desc.hpp: UniqDesc

struct UniqDescHost {   // UniqDesc as the host reads it (runs of equal hashes over different bytes)
    uint64_t off, h0;
    uint32_t d0, sumq;
    uint16_t nlen, slen, qlen, qrel;
};
static_assert(sizeof(UniqDescHost) == kUniqDescBytes, "UniqDesc layout");
}  // namespace hpn

struct hpn_uniq_work {   // what a new session must not inherit: the stage's arrays, the output and what is cached of it
    hpn::Scratch hash, order, djb, sumq, flag, gid, count, best, first, rep, mark, rank, key, val, key_tmp, val_tmp, hist, offs, status,
        list_table, list_key, size, off, out;
    uint32_t N = 0, U = 0;
    uint64_t out_total = 0;
    int cached_which = -1, cached_mate = -1;
};

struct hpn_uniq_state : hpn::FamilyState, hpn_uniq_work {
    static constexpr int kSlot = hpn::kStUniq;
    hpn::StoreSession s;
    int paired = 0;   // s.n_streams - 1
    uint32_t hash_bits = 0;
};

namespace hpn {

inline uint32_t *uniq_kinfo(hpn_uniq_state *u) { return u->s.info.d + kUiBase; }

inline void uniq_drop_session(hpn_uniq_state *u)
{
    session_drop(u->s);
    static_cast<hpn_uniq_work &>(*u) = hpn_uniq_work();
}

// _begin of the three families that group: the session's, and the grouping hash's width
inline int uniq_begin(hpn_ctx *c, hpn_uniq_state *u, int paired, uint64_t max_bytes, uint32_t hash_bits)
{
    const int rc = session_begin(c, u->s, paired ? 2 : 1, max_bytes);
    u->paired = paired ? 1 : 0, u->hash_bits = hash_bits;
    return rc;
}

// the work space of one sort of n pairs (kernels/radix_sort.hpp: SortSpace)
inline int uniq_sort_space(hpn_ctx *c, hpn_uniq_state *u, uint32_t n)
{
    int rc;
    const uint64_t hw = uniq_sort_hist_words(n);
    if ((rc = need(c, u->key_tmp, (size_t)n * 8)) != HPN_OK || (rc = need(c, u->val_tmp, (size_t)n * 4)) != HPN_OK ||
        (rc = need(c, u->hist, hw * 4)) != HPN_OK || (rc = need(c, u->offs, hw * 4)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(hw > n ? hw : n) * 8)) != HPN_OK)
        return rc;
    return HPN_OK;
}

inline int uniq_sort(hpn_ctx *c, hpn_uniq_state *u, uint64_t *keys, uint32_t *vals, uint32_t n, int begin_bit, int end_bit)
{
    int rc;
    if ((rc = uniq_sort_space(c, u, n)) != HPN_OK) return rc;
    HPN_HIP(c, uniq_sort_pairs(keys, vals, n, begin_bit, end_bit, (uint64_t *)u->key_tmp.p, (uint32_t *)u->val_tmp.p, (uint32_t *)u->hist.p,
                               (uint32_t *)u->offs.p, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
    return HPN_OK;
}

// Runs of equal grouping hashes that hold different keys: ordered by their bytes on the host (stable, so equal keys stay in
// file order and lie side by side).  With 64 bits such runs are vanishingly rare; with hash_bits they are the rule.
inline int uniq_order_clashing_runs(hpn_ctx *c, hpn_uniq_state *u)
{
    const uint32_t N = u->N;
    std::vector<uint8_t> text[2];
    std::vector<UniqDescHost> desc[2];
    for (int k = 0; k <= u->paired; ++k) {
        text[k].resize(u->s.m[k].len + 1);
        desc[k].resize(N ? N : 1);
        if (u->s.m[k].len) HPN_HIP(c, hipMemcpy(text[k].data(), (const uint8_t *)u->s.m[k].store.p + kStorePad, u->s.m[k].len, hipMemcpyDeviceToHost));
        HPN_HIP(c, hipMemcpy(desc[k].data(), u->s.m[k].desc.p, (size_t)N * kUniqDescBytes, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> hash(N);
    std::vector<uint32_t> order(N);
    HPN_HIP(c, hipMemcpy(hash.data(), u->hash.p, (size_t)N * 8, hipMemcpyDeviceToHost));
    HPN_HIP(c, hipMemcpy(order.data(), u->order.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    auto key = [&](uint32_t r) {
        std::string s;
        for (int k = 0; k <= u->paired; ++k) {
            const UniqDescHost &d = desc[k][r];
            s.append((const char *)text[k].data() + d.off + d.nlen + 1, d.slen);
        }
        return s;
    };
    for (uint32_t a = 0; a < N;) {
        uint32_t b = a + 1;
        while (b < N && hash[b] == hash[a]) ++b;
        if (b - a > 1) {
            std::vector<std::pair<std::string, uint32_t>> run;
            run.reserve(b - a);
            for (uint32_t i = a; i < b; ++i) run.emplace_back(key(order[i]), order[i]);
            std::stable_sort(run.begin(), run.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
            for (uint32_t i = a; i < b; ++i) order[i] = run[i - a].second;
        }
        a = b;
    }
    HPN_HIP(c, hipMemcpy(u->order.p, order.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    return HPN_OK;
}

// The mates' names of a paired session, ordinal by ordinal (launch_uniq_names): *N -- mate 0's records on entry -- becomes the
// pairs that count, *unmatched the first ordinal whose mate is named otherwise or missing (the caller's -1 stays: none) and
// unmatched_name mate 0's name there.  A single-end session is left as it is.
inline int uniq_match_mates(hpn_ctx *c, hpn_uniq_state *u, uint32_t *N, int64_t *unmatched, char *unmatched_name)
{
    if (!u->paired) return HPN_OK;
    int rc;
    const uint8_t *t0 = u->s.text(0);
    const void *d0 = u->s.m[0].desc.p;
    const uint32_t n2 = (uint32_t)u->s.m[1].n, both = *N < n2 ? *N : n2;
    HPN_HIP(c, hipMemsetAsync(u->s.info.d + kUiFirstBad, 0xff, sizeof(uint32_t), c->stream));
    HPN_HIP(c, launch_uniq_names(t0, d0, u->s.text(1), u->s.m[1].desc.p, both, u->s.info.d + kUiFirstBad, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    if (u->s.info.h[kUiFirstBad] != 0xffffffffu) *N = u->s.info.h[kUiFirstBad], *unmatched = *N;
    else if (*N > n2) *N = n2, *unmatched = n2;   // the mate is missing
    if (*unmatched >= 0) {
        UniqDescHost d;
        HPN_HIP(c, hipMemcpy(&d, (const uint8_t *)d0 + (size_t)*N * kUniqDescBytes, kUniqDescBytes, hipMemcpyDeviceToHost));
        HPN_HIP(c, hipMemcpy(unmatched_name, t0 + d.off, d.nlen, hipMemcpyDeviceToHost));
        unmatched_name[d.nlen] = 0;
    }
    return HPN_OK;
}

// The grouping stage over the u->N records (pairs) of the session, the info block zeroed by the caller.  Leaves: order[] -- the record
// ordinals sorted stably by grouping hash (clashing runs by their bytes), so a group's members are adjacent and ascending; flag[]
// (1 where a group opens), gid[] (its exclusive scan), and per group count, first, rep; u->U; list_table[] and, single-end,
// list_key[]: the groups in the order of the table walk and in sdscmp order.
inline int uniq_group(hpn_ctx *c, hpn_uniq_state *u, bool replace_doubles, uint64_t *hash_size, uint64_t *hash_clashes)
{
    int rc;
    const int paired = u->paired;
    const uint32_t N = u->N;
    const uint8_t *t0 = (const uint8_t *)u->s.m[0].store.p + kStorePad, *t1 = paired ? (const uint8_t *)u->s.m[1].store.p + kStorePad : nullptr;
    const void *d0 = u->s.m[0].desc.p, *d1 = paired ? u->s.m[1].desc.p : nullptr;
    if ((rc = need(c, u->hash, (size_t)N * 8)) != HPN_OK || (rc = need(c, u->order, (size_t)N * 4)) != HPN_OK ||
        (rc = need(c, u->djb, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->sumq, (size_t)N * 4)) != HPN_OK ||
        (rc = need(c, u->flag, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->gid, ((size_t)N + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->mark, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->rank, ((size_t)N + 1) * 4)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK)
        return rc;
    uint64_t *hash = (uint64_t *)u->hash.p;
    uint32_t *order = (uint32_t *)u->order.p, *djb = (uint32_t *)u->djb.p, *sumq = (uint32_t *)u->sumq.p, *flag = (uint32_t *)u->flag.p;
    uint32_t *gid = (uint32_t *)u->gid.p, *mark = (uint32_t *)u->mark.p, *rank = (uint32_t *)u->rank.p;
    uint32_t *ticket = u->s.info.ticket(), *err = u->s.info.err();
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTally], c->stream));
    const uint64_t mask = u->hash_bits ? (1ull << u->hash_bits) - 1 : ~0ull;
    HPN_HIP(c, launch_uniq_pair(t0, d0, t1, d1, paired, N, mask, hash, order, djb, sumq, uniq_kinfo(u), c->stream));
    if ((rc = uniq_sort(c, u, hash, order, N, 0, u->hash_bits ? (int)u->hash_bits : 64)) != HPN_OK) return rc;
    HPN_HIP(c, launch_uniq_flags(t0, d0, t1, d1, paired, hash, order, N, flag, uniq_kinfo(u), c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    *hash_clashes = u->s.info.h[kUiClash];
    const uint32_t max_len = u->s.info.h[kUiMaxLen];
    if (u->s.info.h[kUiClash]) {
        if ((rc = uniq_order_clashing_runs(c, u)) != HPN_OK) return rc;
        HPN_HIP(c, launch_uniq_flags(t0, d0, t1, d1, paired, hash, order, N, flag, uniq_kinfo(u), c->stream));
    }
    if ((rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, uniq_scan32(flag, gid, N, (u64 *)u->status.p, ticket, err, c->stream));
    uint32_t U = 0;
    HPN_HIP(c, hipMemcpyAsync(&U, gid + N, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    u->U = U;
    if ((rc = need(c, u->count, (size_t)U * 4)) != HPN_OK || (rc = need(c, u->best, (size_t)U * 8)) != HPN_OK ||
        (rc = need(c, u->first, (size_t)U * 4)) != HPN_OK || (rc = need(c, u->rep, (size_t)U * 4)) != HPN_OK ||
        (rc = need(c, u->key, (size_t)U * 8)) != HPN_OK || (rc = need(c, u->val, (size_t)U * 4)) != HPN_OK ||
        (rc = need(c, u->list_table, (size_t)U * 4)) != HPN_OK || (rc = need(c, u->list_key, (size_t)U * 4)) != HPN_OK)
        return rc;
    uint32_t *first = (uint32_t *)u->first.p;
    uint64_t *key = (uint64_t *)u->key.p;
    uint32_t *val = (uint32_t *)u->val.p;
    HPN_HIP(c, launch_uniq_reduce(order, flag, gid, sumq, N, U, (uint32_t *)u->count.p, (uint64_t *)u->best.p, first, (uint32_t *)u->rep.p,
                                  uniq_kinfo(u), c->stream));
    HPN_HIP(c, launch_uniq_mark(first, U, mark, N, c->stream));
    HPN_HIP(c, uniq_scan32(mark, rank, N, (u64 *)u->status.p, ticket, err, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    // the table's size and the parity of its doublings
    auto epoch = [](uint32_t j) { return j < 4 ? 0u : (uint32_t)(31 - __builtin_clz(j)) - 1u; };
    uint64_t S = 0;
    uint32_t K = 0;
    if (U) {
        S = 4;
        while (S < U) S *= 2;
        K = epoch(U - 1);
        if (replace_doubles && U >= 4 && (U & (U - 1)) == 0 && u->s.info.h[kUiBehind]) S *= 2, K += 1;
    }
    *hash_size = S;
    int slot_bits = 0;
    while (S && (1ull << slot_bits) < S) ++slot_bits;
    HPN_HIP(c, launch_uniq_table_key(first, rank, djb, U, S ? (uint32_t)(S - 1) : 0u, K, key, val, c->stream));
    if ((rc = uniq_sort(c, u, key, val, U, 0, 32 + slot_bits)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(u->list_table.p, val, (size_t)U * 4, hipMemcpyDeviceToDevice, c->stream));
    if (!paired) {   // sdscmp order: least significant 8-byte word first, every round a stable sort
        HPN_HIP(c, launch_uniq_iota(U, val, c->stream));
        for (uint32_t w = (max_len + 7) / 8; w-- > 0;) {
            HPN_HIP(c, launch_uniq_seq_word(t0, d0, first, val, U, w, key, c->stream));
            if ((rc = uniq_sort(c, u, key, val, U, 0, 64)) != HPN_OK) return rc;
        }
        HPN_HIP(c, hipMemcpyAsync(u->list_key.p, val, (size_t)U * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTally], c->stream));
    c->ev_valid[kFamTally] = true;
    return u->s.info.fetch(c);
}

}  // namespace hpn
