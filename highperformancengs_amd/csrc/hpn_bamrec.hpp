// hpn_bamrec.hpp -- what the BAM sessions keep and do alike, next to the cuts themselves (hpn_cuts.hpp):
//   BadRecord   the first record outside a family's domain, fetched and reported in one place (split, bai and the four below);
//   BamStore    the records of every batch behind one another on the device, with each one's size and place;
//   SliceOut    the stored records in the order a family decided, handed back slice by slice: gathered behind the block the
//               slice before left open, cut as bam_write1 would, CRC-32, for level 0 the stored image.  A family whose output
//               records are not the stored ones byte for byte (fixmate) gives `extra` -- output record j takes
//               size[order[j]] + extra[order[j]] bytes -- and `patch`, which runs on the gathered slice in front of the cuts and
//               the CRC-32; without the two the slices are what they were;
//   RecSession  the three and the life cycle around them (sort, rmdup, merge, fixmate, view): _begin, batches until _finish, then the
//               output's slices; a record outside the domain kills the session and every later call says so.  rec_live is the one
//               check of that cycle, rec_add the batch around a family's kernel, rec_finish_open the head of _finish, and
//               rec_order / rec_emit / rec_blocks / rec_payload / rec_stored the bodies behind a finished session's calls.
// A family writes its _begin, its per-record kernel (size[], soff[] and info words [0..2], see kInfoBad), the middle of its
// _finish, which sets `order` and `n_out`, and every extern "C" function under its own name as a forward.  Plain movable values:
// a session resets by assigning fresh ones.
#pragma once
#include <string.h>

#include <initializer_list>
#include <vector>

#include "hpn_cuts.hpp"
#include "hpn_store.hpp"
#include "kernels/bam_sort.hpp"

namespace hpn {

struct BadRecord {
    int64_t record = -1;
    int32_t tid = 0, pos = 0;
    uint32_t reason = 0;
};

template <class Out>      // (the info and result structs of include/hpngs.h name the four alike)
inline void bad_report(const BadRecord &b, Out *out)
{
    out->bad_record = b.record, out->bad_tid = b.tid, out->bad_pos = b.pos, out->reason = b.reason;
}

// The record the device names, `ord` since _begin and the (ord - base)-th of the batch hpn_bam_raw_index_dev indexed last:
// its refID and pos for the caller's message.
inline int bad_from_batch(hpn_ctx *c, const uint8_t *d_raw, uint64_t ord, uint64_t base, uint32_t reason, BadRecord &bad)
{
    uint64_t off = 0;
    int32_t f[2] = {0, 0};
    HPN_HIP(c, hipMemcpyAsync(&off, (const uint64_t *)c->r_off.p + (ord - base), sizeof off, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    HPN_HIP(c, hipMemcpyAsync(f, d_raw + off + 4, sizeof f, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    bad.record = (int64_t)ord, bad.tid = f[0], bad.pos = f[1], bad.reason = reason;
    return HPN_OK;
}

constexpr uint64_t kMaxRecords = (1ull << 31) - 1;     // a store's contract; the reason a family reports at the cap is its own:
enum { kBsrRecords = 3, kBmrRecords = 2 };             // sort's and merge's (include/hpngs.h; rmdup's kRsRecords, fixmate's kFxrRecords)

struct BamStore {
    Scratch store, size, soff;       // the records' bytes; by ordinal: 4 + block_size, where the record lies in `store`
    uint64_t records = 0, len = 0;
};

// room in size[] and soff[] for n more records (the family's kernel fills them from ordinal st.records on, soff from st.len on)
inline int bamstore_grow(hpn_ctx *c, BamStore &st, uint64_t n)
{
    const uint64_t have = st.records, all = have + n;
    const int rc = grow_keep(c, st.size, all * 4, have * 4);
    return rc != HPN_OK ? rc : grow_keep(c, st.soff, all * 8, have * 8);
}

// The batch's n records, bytes [first, end) of d_raw, go behind the store's by one copy.
inline int bamstore_append(hpn_ctx *c, BamStore &st, const uint8_t *d_raw, uint64_t first, uint64_t end, uint64_t n, const char *who)
{
    if (end < first) return fail(c, HPN_E_HIP, "%s: the batch's records end at %llu, in front of their start %llu", who, (unsigned long long)end,
                                 (unsigned long long)first);
    const uint64_t rec_bytes = end - first;
    const int rc = grow_keep(c, st.store, st.len + rec_bytes + 64, st.len);
    if (rc != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync((uint8_t *)st.store.p + st.len, d_raw + first, rec_bytes, hipMemcpyDeviceToDevice, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (the caller's d_raw is free to go)
    st.len += rec_bytes, st.records += n;
    return HPN_OK;
}

struct SliceOut {
    Scratch psize, out_off, cut_info, Q, ikey, pay, keep;
    CutWork cw;
    uint32_t fill = 0;               // bytes of the open block (in `keep`)
    uint64_t emitted = 0, payload = 0;
    bool ended = false, stored_made = false;
    std::vector<hpn_split_block> list;   // the closed blocks of the last sliceout_emit
    uint64_t payload_bytes = 0, stored_bytes = 0;
    // by stored ordinal: the bytes a record grows by behind its stored ones (nullptr: none), `grown` their sum over the output
    const uint32_t *extra = nullptr;
    uint64_t grown = 0;
    // the slice's records [first, first + cnt) lie gathered at pay, record first + k at out_off[first + k] - out_off[first]:
    // rewrite them in place, on the context's stream (nullptr: they stay as the store has them)
    int (*patch)(hpn_ctx *c, void *arg, const uint32_t *order, const u64 *out_off, uint64_t first, uint64_t cnt, uint8_t *pay) = nullptr;
    void *patch_arg = nullptr;
};

inline int sliceout_begin(hpn_ctx *c, SliceOut &o)
{
    const int rc = scratch_reserve(c, o.cut_info, 64);
    return rc != HPN_OK ? rc : scratch_reserve(c, o.keep, kCutFull + 64);
}

inline int sliceout_reserve(hpn_ctx *c, SliceOut &o, uint64_t n_in)      // room for the offsets of a session of n_in records
{
    const int rc = need(c, o.psize, n_in * 4);
    return rc != HPN_OK ? rc : need(c, o.out_off, (n_in + 1) * 8);
}

// out_off[j]: where output record j = stored record order[j] starts in the output's payload; out_off[n_out] = o.payload, which is
// the store's length and what the records grow by (exact) or no more than it.  sliceout_reserve has been called.
inline int sliceout_offsets(hpn_ctx *c, SliceOut &o, const BamStore &st, const uint32_t *order, uint64_t n_out, bool exact, const char *who)
{
    if (o.extra) HPN_HIP(c, launch_bamsort_psize_grown((const uint32_t *)st.size.p, o.extra, order, n_out, (uint32_t *)o.psize.p, c->stream));
    else HPN_HIP(c, launch_bamsort_psize((const uint32_t *)st.size.p, order, n_out, (uint32_t *)o.psize.p, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    const int rc = hpn_excl_scan(c, n_out ? o.psize.p : nullptr, 32, o.out_off.p, 64, n_out);
    if (rc != HPN_OK) return rc;
    HPN_HIP(c, hipMemcpyAsync(&o.payload, (const u64 *)o.out_off.p + n_out, 8, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (exact ? o.payload != st.len + o.grown : o.payload > st.len + o.grown)
        return fail(c, HPN_E_HIP, "%s: the %s records take %llu bytes, the store holds %llu", who, exact ? "sorted" : "surviving", (unsigned long long)o.payload,
                    (unsigned long long)(st.len + o.grown));
    return HPN_OK;
}

// The next slice of the n_out output records: gathered behind the open block's bytes, cut, the last block kept open unless
// `last`, every closed block with its CRC-32.
inline int sliceout_emit(hpn_ctx *c, SliceOut &o, const BamStore &st, const uint32_t *order, uint64_t n_out, uint64_t first_record, uint64_t max_records,
                         int last, hpn_split_info *info, const char *who)
{
    if (o.ended) return fail(c, HPN_E_STATE, "%s_emit behind the call that ended the file", who);
    if (first_record != o.emitted)
        return fail(c, HPN_E_ARG, "%s_emit: slice from record %llu, the next one is %llu (the open block is carried from slice to slice)", who,
                    (unsigned long long)first_record, (unsigned long long)o.emitted);
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    info->bad_record = -1, info->tid_first = 0, info->tid_last = -1;
    o.list.clear(), o.payload_bytes = 0, o.stored_bytes = 0, o.stored_made = false;
    const uint64_t left = n_out - first_record, cnt = max_records < left ? max_records : left;
    if (cnt > 0xfffffff0ull) return fail(c, HPN_E_ARG, "more than 2^32 records in one slice");
    if (last && cnt != left) return fail(c, HPN_E_ARG, "%s_emit: last = 1 with %llu records behind the slice", who, (unsigned long long)(left - cnt));
    info->n_records = cnt;
    const uint64_t m = cnt + 1;
    int rc;
    u64 span[2] = {0, 0};      // the slice's bytes in the output's payload
    if (cnt) {
        HPN_HIP(c, hipMemcpyAsync(&span[0], (const u64 *)o.out_off.p + first_record, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipMemcpyAsync(&span[1], (const u64 *)o.out_off.p + first_record + cnt, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (span[1] < span[0] || span[1] > o.payload) return fail(c, HPN_E_HIP, "%s: the slice's offsets are out of order", who);
    }
    const uint64_t rec_bytes = span[1] - span[0], total = o.fill + rec_bytes;
    if ((rc = scratch_reserve(c, o.Q, (m + 1) * sizeof(u64))) != HPN_OK || (rc = scratch_reserve(c, o.ikey, (m + 1) * sizeof(uint32_t))) != HPN_OK ||
        (rc = cut_reserve(c, o.cw, m)) != HPN_OK || (rc = scratch_reserve(c, o.pay, total + 64)) != HPN_OK)
        return rc;
    const u64 init[4] = {~0ull, 0, 0, 0};
    HPN_HIP(c, hipMemcpyAsync(o.cut_info.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    if (o.fill) HPN_HIP(c, hipMemcpyAsync(o.pay.p, o.keep.p, o.fill, hipMemcpyDeviceToDevice, c->stream));
    HPN_HIP(c, launch_bamsort_items((const u64 *)o.out_off.p, first_record, cnt, o.fill, o.fill ? 0u : kCutNoKey, (u64 *)o.Q.p, (uint32_t *)o.ikey.p,
                                    c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_bamsort_gather((const uint8_t *)st.store.p, (const u64 *)st.soff.p, (const uint32_t *)st.size.p, order, (const u64 *)o.out_off.p,
                                     first_record, cnt, (uint8_t *)o.pay.p + o.fill, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    if (o.patch && cnt && (rc = o.patch(c, o.patch_arg, order, (const u64 *)o.out_off.p, first_record, cnt, (uint8_t *)o.pay.p + o.fill)) != HPN_OK) return rc;
    HPN_HIP(c, hipStreamSynchronize(c->stream));       // (`init` is this call's)
    if ((rc = cut_blocks(c, o.cw, (const u64 *)o.Q.p, (const uint32_t *)o.ikey.p, m, 1, (u64 *)o.cut_info.p, total, o.list, who)) != HPN_OK) return rc;
    int32_t open_tid = -1;
    if ((rc = carry_open(c, o.keep, (const uint8_t *)o.pay.p, o.list, total, last != 0, &o.fill, &open_tid)) != HPN_OK) return rc;
    if (last) o.ended = true;
    if ((rc = close_blocks(c, o.cw, (const uint8_t *)o.pay.p, o.list, false, &o.payload_bytes, &o.stored_bytes)) != HPN_OK) return rc;
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    o.emitted += cnt;
    info->n_blocks = o.list.size(), info->payload_bytes = o.payload_bytes, info->open_bytes = o.fill;
    if (!o.list.empty()) info->tid_first = info->tid_last = 0;
    return HPN_OK;
}

inline int sliceout_payload(const SliceOut &o, const uint8_t **d_payload, uint64_t *n_bytes)
{
    *d_payload = (const uint8_t *)o.pay.p, *n_bytes = o.payload_bytes;
    return HPN_OK;
}

// (made when it is asked for: only a level-0 writer wants it)
inline int sliceout_stored(hpn_ctx *c, SliceOut &o, const uint8_t **d_image, uint64_t *n_bytes)
{
    HPN_HIP(c, hipSetDevice(c->device));
    if (!o.stored_made) {
        const int rc = stored_image(c, o.cw, (const uint8_t *)o.pay.p, o.list, &o.stored_bytes);
        if (rc != HPN_OK) return rc;
        o.stored_made = true;
    }
    *d_image = (const uint8_t *)o.cw.img.p, *n_bytes = o.stored_bytes;
    return HPN_OK;
}

// ---- the session around the three ----
// Words 0, 1, 2 of every family's info array, whatever else it keeps there: the lowest (ordinal << bits | reason) of a record outside
// the domain (~0: none), and where in the inflated stream the batch's first record starts and its last one ends.
enum { kInfoBad = 0, kInfoFirst = 1, kInfoEnd = 2, kInfoHead = 3 };
static_assert(kBsBad == kInfoBad && kBsFirst == kInfoFirst && kBsEnd == kInfoEnd, "k_sort_keys' info words are the sessions'");

struct RecSession {        // what a new session must not inherit: _begin assigns a fresh one
    BamStore st;
    SliceOut out;
    Scratch info;
    bool open = false, dead = false, finished = false;
    BadRecord bad;
    const uint32_t *order = nullptr;     // the output: record j is stored record order[j], j < n_out (the family's _finish sets both)
    uint64_t n_out = 0;
};

// A state type U derives from FamilyState and RecSession and names itself: kName ("hpn_bam_sort"), kVerb (what _finish does to
// the records: "sorted") and wrong_count(c, who, n, want), the refusal of n entries asked for where the session has `want`.
enum RecWant { kRecFeeding, kRecFinishing, kRecFinished };       // a call in front of _finish, _finish itself, a call behind it

template <class U>
inline U *rec_live(hpn_ctx *c, const char *who, RecWant want)
{
    U *u = state<U>(c);
    if (!u || !u->open) return fail(c, HPN_E_STATE, "%s before %s_begin", who, U::kName), nullptr;
    if (want == kRecFinished) {
        if (!u->finished) return fail(c, HPN_E_STATE, "%s before %s_finish", who, U::kName), nullptr;
        if (u->dead) return fail(c, HPN_E_STATE, "%s: a record lies outside the domain, nothing was %s", who, U::kVerb), nullptr;
    } else if (u->finished) {
        if (want == kRecFinishing) return fail(c, HPN_E_STATE, "%s twice", who), nullptr;
        return fail(c, HPN_E_STATE, "%s behind %s_finish", who, U::kName), nullptr;
    }
    return u;
}

struct ByOrdinal {         // an array a family keeps by ordinal and grows batch by batch, and its entry's bytes
    Scratch *s;
    uint32_t width;
};

// how most kernels pack word kInfoBad: 3 reason bits; refID and pos from the batch
template <class U>
inline int rec_bad_of_batch(hpn_ctx *c, U &u, const uint8_t *d_raw, u64 word, uint64_t base)
{
    return bad_from_batch(c, d_raw, word >> 3, base, (uint32_t)(word & 7), u.bad);
}

// One indexed batch (hpn_bam_raw_index_dev's last) into a live session: arrays[] and the store's grown, launch(n, base) -- the
// family's kernel over the batch's n records, ordinals base.. --, then the records appended, or the session killed by the first
// record outside the domain, which bad_of(c, u, d_raw, word, base) makes of word kInfoBad, or by the cap, with cap_reason.
template <class U, class Info, class Launch, class BadOf>
inline int rec_add(hpn_ctx *c, U &u, const uint8_t *d_raw, Info *info, uint32_t cap_reason, std::initializer_list<ByOrdinal> arrays, Launch &&launch,
                   BadOf &&bad_of)
{
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t n = d_raw ? c->r_n : 0;
    BamStore &st = u.st;
    auto report = [&]() { info->n_records = n, info->store_bytes = st.len, bad_report(u.bad, info); };
    report();
    if (u.dead || !n) return HPN_OK;
    if (st.records + n > kMaxRecords) {                // the first record the session cannot take
        u.dead = true;
        u.bad.record = (int64_t)kMaxRecords, u.bad.reason = cap_reason;
        st.records += n;
        report();
        return HPN_OK;
    }
    int rc;
    const uint64_t have = st.records, all = have + n;
    for (const ByOrdinal &a : arrays)
        if ((rc = grow_keep(c, *a.s, all * a.width, have * a.width)) != HPN_OK) return rc;
    if ((rc = bamstore_grow(c, st, n)) != HPN_OK) return rc;
    HPN_HIP(c, launch(n, have));
    u64 h[kInfoHead];
    HPN_HIP(c, hipMemcpyAsync(h, u.info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (h[kInfoBad] != ~0ull) {                        // the first record outside the domain: refID and pos for the message
        if ((rc = bad_of(c, u, d_raw, h[kInfoBad], have)) != HPN_OK) return rc;
        u.dead = true;
        st.records = all;
        report();
        return HPN_OK;
    }
    if ((rc = bamstore_append(c, st, d_raw, h[kInfoFirst], h[kInfoEnd], n, U::kName)) != HPN_OK) return rc;
    report();
    return HPN_OK;
}

// The head of _finish.  u == nullptr behind it: return what it returned -- a refusal, or HPN_OK for a session a record has killed,
// which *res says.  more(u, res): what the family's result holds beside n_records and the bad record, whether the session lives or not.
template <class U, class Res, class More>
inline int rec_finish_open(hpn_ctx *c, const char *who, Res *res, U *&u, More &&more)
{
    u = nullptr;
    if (!c || !res) return HPN_E_ARG;
    U *s = rec_live<U>(c, who, kRecFinishing);
    if (!s) return HPN_E_STATE;
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->n_records = s->st.records;
    bad_report(s->bad, res);
    more(*s, res);
    s->finished = true;
    if (!s->dead) u = s;
    return HPN_OK;
}

template <class U, class Res>
inline int rec_finish_open(hpn_ctx *c, const char *who, Res *res, U *&u)
{
    return rec_finish_open(c, who, res, u, [](U &, Res *) {});
}

// src[0..n) of a finished session to the host (the caller has held n to what the session has: U::wrong_count says the refusal)
inline int rec_copy_out(hpn_ctx *c, uint32_t *dst, const void *src, uint64_t n)
{
    if (!n) return HPN_OK;
    HPN_HIP(c, hipSetDevice(c->device));
    HPN_HIP(c, hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

template <class U>
inline int rec_order(hpn_ctx *c, const char *who, uint32_t *order, uint64_t n)
{
    if (!c || (n && !order)) return HPN_E_ARG;
    U *u = rec_live<U>(c, who, kRecFinished);
    if (!u) return HPN_E_STATE;
    return n != u->n_out ? U::wrong_count(c, who, n, u->n_out) : rec_copy_out(c, order, u->order, n);
}

template <class U>
inline int rec_emit(hpn_ctx *c, const char *who, uint64_t first_record, uint64_t max_records, int last, hpn_split_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    U *u = rec_live<U>(c, who, kRecFinished);
    return !u ? HPN_E_STATE : sliceout_emit(c, u->out, u->st, u->order, u->n_out, first_record, max_records, last, info, U::kName);
}

template <class U>
inline int rec_blocks(hpn_ctx *c, const char *who, uint64_t first, hpn_split_block *out, uint64_t cap, uint64_t *n)
{
    if (!c || !n) return HPN_E_ARG;
    U *u = rec_live<U>(c, who, kRecFinished);
    return !u ? HPN_E_STATE : list_blocks(c, u->out.list, first, out, cap, n);
}

template <class U>
inline int rec_payload(hpn_ctx *c, const char *who, const uint8_t **d_payload, uint64_t *n_bytes)
{
    if (!c || !d_payload || !n_bytes) return HPN_E_ARG;
    U *u = rec_live<U>(c, who, kRecFinished);
    return !u ? HPN_E_STATE : sliceout_payload(u->out, d_payload, n_bytes);
}

template <class U>
inline int rec_stored(hpn_ctx *c, const char *who, const uint8_t **d_image, uint64_t *n_bytes)
{
    if (!c || !d_image || !n_bytes) return HPN_E_ARG;
    U *u = rec_live<U>(c, who, kRecFinished);
    return !u ? HPN_E_STATE : sliceout_stored(c, u->out, d_image, n_bytes);
}

}  // namespace hpn
