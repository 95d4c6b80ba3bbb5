// hpn_mrle.hip -- C ABI of gzfastq_mrle.c: hpn_mrle_begin / _add / _finish / _write.  Kernels: kernels/mrle.hip, the framing of
// kernels/fastq_sort.hip (k_sort_frame, as it is), the 64-bit scan of kernels/fastq_uniq.hip, the line index of
// kernels/fastq_text.hip.  The store and its session: hpn_store.hpp.
//
// The session is hpn_fastq_sort_*'s front half -- the whole text in the store, one SortDesc per record -- with another back half:
// the encoded sizes and the lines' lengths, two scans, the encoder, the decoder over what the encoder wrote, and the layout of
// the two streams on one descriptor.  The host walks no record: it sees three totals and the domain word.
#include "hpn_store.hpp"
#include "kernels/sort_desc.hpp"

namespace hpn {
// kernels/mrle.hip
hipError_t launch_mrle_sizes(const uint8_t *d_text, const void *d_desc, uint32_t n, uint32_t *d_psize, uint32_t *d_tsize, uint8_t *d_flag,
                             uint32_t *d_bad, int n_cu, hipStream_t st);
hipError_t launch_mrle_write(const uint8_t *d_text, const void *d_desc, const uint64_t *d_poff, const uint8_t *d_flag, uint32_t n,
                             uint8_t *d_packed, int n_cu, hipStream_t st);
hipError_t launch_mrle_decode(const uint8_t *d_packed, const uint64_t *d_poff, const uint64_t *d_toff, uint32_t n, uint8_t *d_text_out, int n_cu,
                              hipStream_t st);
uint64_t mrle_shared_bytes(uint64_t packed_total, uint64_t text_total);
hipError_t launch_mrle_shared(const uint8_t *d_packed, const uint64_t *d_poff, uint64_t packed_total, const uint8_t *d_text_out,
                              const uint64_t *d_toff, uint64_t text_total, uint32_t n, uint8_t *d_out, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
enum { kMlBad = kInfoOwn };   // the family's word of the info block
enum { kPacked = HPN_MRLE_PACKED, kText = HPN_MRLE_TEXT, kShared = HPN_MRLE_SHARED };   // (plain names: HPN_HIP quotes its call in the message)
}  // namespace

struct hpn_mrle_work {   // what a new session must not inherit
    Scratch psize, tsize, flag, poff, toff, status, out[3];   // out: by HPN_MRLE_*
    uint64_t out_total[3] = {0, 0, 0};
};

struct hpn_mrle_state : FamilyState, hpn_mrle_work {
    static constexpr int kSlot = kStMrle;
    StoreSession s;
};

namespace {

void drop_session(hpn_mrle_state *u)
{
    session_drop(u->s);
    static_cast<hpn_mrle_work &>(*u) = hpn_mrle_work();
}

}  // namespace

extern "C" {

int hpn_mrle_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_mrle_state *u = state_make<hpn_mrle_state>(c);
    drop_session(u);
    return session_begin(c, u->s, 1, max_bytes);
}

int hpn_mrle_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_mrle_state *u = state<hpn_mrle_state>(c);
    return session_add(c, u ? &u->s : nullptr, "hpn_mrle", 0, kSortDescBytes, frame_by<launch_sort_frame>, nullptr, 4u, text, nbytes, last, false, info);
}

int hpn_mrle_finish(hpn_ctx *c, hpn_mrle_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_mrle_state *u = state<hpn_mrle_state>(c);
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_mrle", kSortDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    res->bad_record = -1;
    const uint32_t N = (uint32_t)u->s.m[0].n;
    res->n_records = N;
    if (!N) {   // no record: three empty outputs
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->s.finished = true;
        return HPN_OK;
    }
    if ((rc = need(c, u->psize, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->tsize, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->flag, N)) != HPN_OK ||
        (rc = need(c, u->poff, ((size_t)N + 1) * 8)) != HPN_OK || (rc = need(c, u->toff, ((size_t)N + 1) * 8)) != HPN_OK)
        return rc;
    const uint8_t *text = u->s.text(0);
    const void *desc = u->s.m[0].desc.p;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_mrle_sizes(text, desc, N, (uint32_t *)u->psize.p, (uint32_t *)u->tsize.p, (uint8_t *)u->flag.p, u->s.info.d + kMlBad, c->n_cu,
                                 c->stream));
    uint64_t total[3] = {0, 0, 0};
    if ((rc = scan_sizes(c, u->s.info, u->status, u->psize, u->poff, N, &total[kPacked])) != HPN_OK) return rc;   // (fetches the info block)
    if (u->s.info.h[kMlBad] != 0xffffffffu) {
        const uint32_t bad = u->s.info.h[kMlBad];
        res->bad_record = (int64_t)bad;
        drop_session(u);
        return fail(c, HPN_E_DOMAIN, "record %u (0-based) has a quality byte outside #/7<BF: the reference indexes an 8-entry table at 255 there", bad);
    }
    if ((rc = scan_sizes(c, u->s.info, u->status, u->tsize, u->toff, N, &total[kText])) != HPN_OK) return rc;
    total[kShared] = mrle_shared_bytes(total[kPacked], total[kText]);
    for (int k = 0; k < 3; ++k)
        if ((rc = need(c, u->out[k], total[k])) != HPN_OK) return rc;
    uint8_t *packed = (uint8_t *)u->out[kPacked].p, *lines = (uint8_t *)u->out[kText].p;
    const uint64_t *poff = (const uint64_t *)u->poff.p, *toff = (const uint64_t *)u->toff.p;
    HPN_HIP(c, launch_mrle_write(text, desc, poff, (const uint8_t *)u->flag.p, N, packed, c->n_cu, c->stream));
    HPN_HIP(c, launch_mrle_decode(packed, poff, toff, N, lines, c->n_cu, c->stream));   // the codec's round trip: from the encoded bytes
    HPN_HIP(c, launch_mrle_shared(packed, poff, total[kPacked], lines, toff, total[kText], N, (uint8_t *)u->out[kShared].p,
                                  c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) u->out_total[k] = res->out_bytes[k] = total[k];
    u->s.finished = true;
    return HPN_OK;
}

int hpn_mrle_write(hpn_ctx *c, int which, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_mrle_state *u = state<hpn_mrle_state>(c);
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_mrle", written);
    if (rc != HPN_OK) return rc;
    if (which < kPacked || which > kShared) return fail(c, HPN_E_ARG, "output %d (0 packed, 1 text, 2 shared)", which);
    return session_write_slice(c, u->out[which], u->out_total[which], offset, out, cap, written);
}

}  // extern "C"
