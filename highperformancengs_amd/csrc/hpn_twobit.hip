// hpn_twobit.hip -- C ABI of the 2-bit pair (fastq2twobit.c, twoBit2seq.c): hpn_twobit_pack_begin / _add / _finish / _write and
// the stateless hpn_twobit_unpack.  Kernels: kernels/twobit.hip, the framing of kernels/fastq_sort.hip (k_sort_frame, as it is),
// the 64-bit scan of kernels/fastq_uniq.hip, the line index of kernels/fastq_text.hip.  The store and its framing in place:
// hpn_store.hpp.
//
// The pack session is hpn_fastq_sort_*'s front half -- the whole text in the store, one SortDesc per record -- with another back
// half: sizes in reverse input order, one scan, one writer.  The whole text stays resident until the output has been fetched;
// packing chunk by chunk, so that only the packed bytes stay, is a follow-up (docs/kernels/twobit.md).
#include "hpn_store.hpp"
#include "kernels/sort_desc.hpp"

namespace hpn {
// kernels/twobit.hip
hipError_t launch_pack_sizes(const void *d_desc, uint32_t n, uint32_t *d_size, hipStream_t st);
hipError_t launch_pack_write(const uint8_t *d_text, const void *d_desc, const uint64_t *d_off, uint32_t n, uint8_t *d_out, uint32_t *d_bad,
                             int n_cu, hipStream_t st);
hipError_t launch_twobit_unpack(const uint8_t *d_packed, uint32_t seq_len, uint32_t packed_len, uint64_t n_records, uint8_t *d_out, int n_cu,
                                hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
enum { kTbBad = kInfoOwn };   // the family's word of the info block
}  // namespace

struct hpn_twobit_work {   // what a new session must not inherit
    Scratch size, off, status, out;
    uint64_t out_total = 0;
};

struct hpn_twobit_state : FamilyState, hpn_twobit_work {
    static constexpr int kSlot = kStTwobit;
    StoreSession s;
};

namespace {

void drop_session(hpn_twobit_state *u)
{
    session_drop(u->s);
    static_cast<hpn_twobit_work &>(*u) = hpn_twobit_work();
}

}  // namespace

extern "C" {

int hpn_twobit_pack_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_twobit_state *u = state_make<hpn_twobit_state>(c);
    drop_session(u);
    return session_begin(c, u->s, 1, max_bytes);
}

int hpn_twobit_pack_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_twobit_state *u = state<hpn_twobit_state>(c);
    return session_add(c, u ? &u->s : nullptr, "hpn_twobit_pack", 0, kSortDescBytes, frame_by<launch_sort_frame>, nullptr, 4u, text, nbytes, last, false, info);
}

int hpn_twobit_pack_finish(hpn_ctx *c, hpn_twobit_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_twobit_state *u = state<hpn_twobit_state>(c);
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_twobit_pack", kSortDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    res->bad_record = -1;
    const uint32_t N = (uint32_t)u->s.m[0].n;
    res->n_records = N;
    if (!N) {   // no record: no header either
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->out_total = 0;
        u->s.finished = true;
        return HPN_OK;
    }
    SortDesc d;   // the input's last record gives the header
    HPN_HIP(c, hipMemcpy(&d, (const SortDesc *)u->s.m[0].desc.p + (N - 1), sizeof d, hipMemcpyDeviceToHost));
    res->seq_len = d.slen & 255u, res->packed_len = ((d.slen + 3u) >> 2) & 255u;
    if ((rc = need(c, u->size, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->off, ((size_t)N + 1) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_pack_sizes(u->s.m[0].desc.p, N, (uint32_t *)u->size.p, c->stream));
    uint64_t sum = 0;
    if ((rc = scan_sizes(c, u->s.info, u->status, u->size, u->off, N, &sum)) != HPN_OK) return rc;
    const uint64_t total = 2u + sum;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, launch_pack_write(u->s.text(0), u->s.m[0].desc.p, (const uint64_t *)u->off.p, N, (uint8_t *)u->out.p, u->s.info.d + kTbBad, c->n_cu,
                                 c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    if (u->s.info.h[kTbBad] != 0xffffffffu) {
        res->bad_record = (int64_t)u->s.info.h[kTbBad];
        drop_session(u);
        return fail(c, HPN_E_DOMAIN, "record %u (0-based) has a sequence byte of 0x80 or more: the reference indexes its table with a signed char there",
                    u->s.info.h[kTbBad]);
    }
    u->out_total = res->out_bytes = total;
    u->s.finished = true;
    return HPN_OK;
}

int hpn_twobit_pack_write(hpn_ctx *c, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_twobit_state *u = state<hpn_twobit_state>(c);
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_twobit_pack", written);
    return rc != HPN_OK ? rc : session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

int hpn_twobit_unpack(hpn_ctx *c, uint32_t seq_len, uint32_t packed_len, const void *packed, uint64_t n_records, void *out, uint64_t out_cap,
                      uint64_t *out_bytes)
{
    if (!c || !out_bytes) return HPN_E_ARG;
    *out_bytes = 0;
    if (seq_len > 255u || packed_len > 255u) return fail(c, HPN_E_ARG, "seq_len %u / packed_len %u: the header holds one byte each", seq_len, packed_len);
    if (!n_records) return HPN_OK;
    if (!packed_len) return fail(c, HPN_E_ARG, "packed_len is 0 (the reference never ends on such a header)");
    if (n_records >= (1ull << 40)) return fail(c, HPN_E_ARG, "%llu records in one call", (unsigned long long)n_records);
    const uint64_t in_bytes = n_records * packed_len, need_bytes = n_records * ((uint64_t)seq_len + 1u);
    *out_bytes = need_bytes;
    if (need_bytes > out_cap) return fail(c, HPN_E_CAPACITY, "the output needs %llu bytes, out_cap is %llu", (unsigned long long)need_bytes, (unsigned long long)out_cap);
    if (!packed || !out) return fail(c, HPN_E_ARG, "packed or out is NULL");
    HPN_HIP(c, hipSetDevice(c->device));
    // host pointers are staged (s_a: the records, s_b: the text); device pointers are used where they lie
    hipPointerAttribute_t at;
    auto on_device = [&](const void *p) {
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return at.type == hipMemoryTypeDevice;
    };
    int rc;
    const uint8_t *d_in = (const uint8_t *)packed;
    uint8_t *d_out = (uint8_t *)out;
    const bool in_dev = on_device(packed), out_dev = on_device(out);
    if (!in_dev) {
        if ((rc = scratch_reserve(c, c->s_a, in_bytes)) != HPN_OK) return rc;
        HPN_HIP(c, hipMemcpyAsync(c->s_a.p, packed, in_bytes, hipMemcpyDefault, c->stream));
        d_in = (const uint8_t *)c->s_a.p;
    }
    if (!out_dev) {
        if ((rc = scratch_reserve(c, c->s_b, need_bytes)) != HPN_OK) return rc;
        d_out = (uint8_t *)c->s_b.p;
    }
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_twobit_unpack(d_in, seq_len, packed_len, n_records, d_out, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    if (!out_dev) HPN_HIP(c, hipMemcpyAsync(out, d_out, need_bytes, hipMemcpyDefault, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

}  // extern "C"
