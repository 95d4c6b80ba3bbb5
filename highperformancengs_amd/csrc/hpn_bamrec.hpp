// hpn_bamrec.hpp -- what the BAM sessions keep and do alike, next to the cuts themselves (hpn_cuts.hpp):
//   BadRecord   the first record outside a family's domain, fetched and reported in one place (split, bai, sort, rmdup);
//   BamStore    the records of every batch behind one another on the device, with each one's size and place (sort, rmdup);
//   SliceOut    the stored records in the order a family decided, handed back slice by slice: gathered behind the block the
//               slice before left open, cut as bam_write1 would, CRC-32, for level 0 the stored image (sort, rmdup).  A family
//               whose output records are not the stored ones byte for byte (fixmate) gives `extra` -- output record j takes
//               size[order[j]] + extra[order[j]] bytes -- and `patch`, which runs on the gathered slice in front of the cuts and
//               the CRC-32; without the two the slices are what they were.
// A family writes its per-record kernel (size[], soff[] and info words [0..2] as k_sort_keys fills them), its _finish and its
// order array.  Plain movable values: a session resets by assigning fresh ones.
#pragma once
#include <string.h>

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

constexpr uint64_t kMaxRecords = (1ull << 31) - 1;     // a store's contract; the reason a family reports at the cap is its own

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

}  // namespace hpn
