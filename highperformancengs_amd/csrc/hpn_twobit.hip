// hpn_twobit.hip -- C ABI of the 2-bit pair (fastq2twobit.c, twoBit2seq.c): hpn_twobit_pack_begin / _add / _finish / _write and
// the stateless hpn_twobit_unpack.  Kernels: kernels/twobit.hip, the framing of kernels/fastq_sort.hip (k_sort_frame, as it is),
// the 64-bit scan of kernels/fastq_uniq.hip, the line index of kernels/fastq_text.hip.  The store and its framing in place:
// hpn_store.hpp.
//
// The pack session is hpn_fastq_sort_*'s front half -- the whole text in the store, one SortDesc per record -- with another back
// half: sizes in reverse input order, one scan, one writer.  The whole text stays resident until the output has been fetched;
// packing chunk by chunk, so that only the packed bytes stay, is a follow-up (docs/kernels/twobit.md).
#include <string.h>

#include "hpn_store.hpp"

namespace hpn {
// kernels/fastq_sort.hip
hipError_t launch_sort_frame(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                             void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st);
// kernels/fastq_uniq.hip
hipError_t uniq_scan64(const uint32_t *d_in, uint64_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st);
uint64_t uniq_scan_tiles(uint64_t n);
// kernels/twobit.hip
hipError_t launch_pack_sizes(const void *d_desc, uint32_t n, uint32_t *d_size, hipStream_t st);
hipError_t launch_pack_write(const uint8_t *d_text, const void *d_desc, const uint64_t *d_off, uint32_t n, uint8_t *d_out, uint32_t *d_bad,
                             int n_cu, hipStream_t st);
hipError_t launch_twobit_unpack(const uint8_t *d_packed, uint32_t seq_len, uint32_t packed_len, uint64_t n_records, uint8_t *d_out, int n_cu,
                                hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
constexpr size_t kDescBytes = 16;                                       // kernels/fastq_sort.hip: SortDesc
enum { kTbTicket = 0, kTbErr = 1, kTbBad = 2, kTbWords = 4 };           // the device's info block (uint32 words)
}  // namespace

struct hpn_twobit_state {
    uint64_t limit = 0;
    bool open = false, finished = false;
    RecordStore m;
    Scratch size, off, status, out;
    uint32_t *d_info = nullptr, *h_info = nullptr;
    uint64_t out_total = 0;
};

namespace {

void drop_session(hpn_twobit_state *u)
{
    store_release(u->m);
    Scratch *ss[] = {&u->size, &u->off, &u->status, &u->out};
    for (Scratch *s : ss) release_scratch(*s);
    u->open = u->finished = false;
    u->out_total = 0;
}

}  // namespace

namespace hpn {
void twobit_release(hpn_ctx *c)
{
    if (!c->tb) return;
    drop_session(c->tb);
    if (c->tb->d_info) (void)hipFree(c->tb->d_info);
    if (c->tb->h_info) (void)hipHostFree(c->tb->h_info);
    delete c->tb;
    c->tb = nullptr;
}
}  // namespace hpn

extern "C" {

int hpn_twobit_pack_begin(hpn_ctx *c, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    if (!c->tb) c->tb = new hpn_twobit_state;
    hpn_twobit_state *u = c->tb;
    if (!u->d_info) {
        HPN_HIP(c, hipMalloc((void **)&u->d_info, kTbWords * sizeof(uint32_t)));
        HPN_HIP(c, hipHostMalloc((void **)&u->h_info, kTbWords * sizeof(uint32_t), hipHostMallocDefault));
    }
    drop_session(u);
    if (!max_bytes) {   // half of what is free, as hpn_fastq_sort_begin: the other half is the reserve for the store's growth and the output
        size_t fr = 0, total = 0;
        HPN_HIP(c, hipMemGetInfo(&fr, &total));
        max_bytes = fr / 2;
    }
    u->limit = max_bytes;
    u->open = true;
    return HPN_OK;
}

int hpn_twobit_pack_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_twobit_state *u = c->tb;
    if (!u || !u->open || u->finished) return fail(c, HPN_E_STATE, "hpn_twobit_pack_begin first (or the session was closed by an irregular chunk)");
    if (nbytes && !text) return fail(c, HPN_E_ARG, "text is NULL");
    RecordStore &m = u->m;
    if (m.closed) return fail(c, HPN_E_STATE, "the stream has had its last chunk");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t span = m.len - m.pos + nbytes;
    if (span >= (1ull << 31) - 4096) return fail(c, HPN_E_ARG, "chunk of %llu bytes (limit 2^31 - 4 KiB with the unfinished record)", (unsigned long long)nbytes);
    if (m.len + nbytes > u->limit) {
        u->open = false;
        return fail(c, HPN_E_CAPACITY, "the store needs %llu bytes, max_bytes is %llu", (unsigned long long)(m.len + nbytes), (unsigned long long)u->limit);
    }
    bool close = false;
    const int rc = store_add(c, m, kDescBytes, launch_sort_frame, text, nbytes, last, &info->n_records, &info->irregular, &close);
    info->store_bytes = m.len;
    if (close) u->open = false;
    return rc;
}

int hpn_twobit_pack_finish(hpn_ctx *c, hpn_twobit_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_twobit_state *u = c->tb;
    if (!u || !u->open || u->finished) return fail(c, HPN_E_STATE, "no open hpn_twobit_pack session");
    if (!u->m.closed) return fail(c, HPN_E_STATE, "the stream needs its last chunk first");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->bad_record = -1;
    int rc;
    const uint32_t N = (uint32_t)u->m.n;
    res->n_records = N;
    if (!N) {   // no record: no header either
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        u->out_total = 0;
        u->finished = true;
        return HPN_OK;
    }
    HPN_HIP(c, hipMemsetAsync(u->d_info, 0, kTbWords * sizeof(uint32_t), c->stream));
    struct {
        uint64_t off;
        uint16_t nlen, slen, qlen, qrel;
    } d;   // SortDesc as the host reads it: the input's last record gives the header
    static_assert(sizeof d == kDescBytes, "SortDesc layout");
    HPN_HIP(c, hipMemcpy(&d, (const uint8_t *)u->m.desc.p + (size_t)(N - 1) * kDescBytes, kDescBytes, hipMemcpyDeviceToHost));
    res->seq_len = d.slen & 255u, res->packed_len = ((d.slen + 3u) >> 2) & 255u;
    if ((rc = need(c, u->size, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->off, ((size_t)N + 1) * 8)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_pack_sizes(u->m.desc.p, N, (uint32_t *)u->size.p, c->stream));
    HPN_HIP(c, uniq_scan64((const uint32_t *)u->size.p, (uint64_t *)u->off.p, N, (u64 *)u->status.p, u->d_info + kTbTicket, u->d_info + kTbErr, c->stream));
    uint64_t sum = 0;
    HPN_HIP(c, hipMemcpyAsync(&sum, (const uint64_t *)u->off.p + N, 8, hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t total = 2u + sum;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, launch_pack_write((const uint8_t *)u->m.store.p + kStorePad, u->m.desc.p, (const uint64_t *)u->off.p, N, (uint8_t *)u->out.p,
                                 u->d_info + kTbBad, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    HPN_HIP(c, hipMemcpyAsync(u->h_info, u->d_info, kTbWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (u->h_info[kTbErr]) return fail(c, HPN_E_HIP, "prefix-scan hand-off timed out");
    if (u->h_info[kTbBad] != 0xffffffffu) {
        res->bad_record = (int64_t)u->h_info[kTbBad];
        drop_session(u);
        return fail(c, HPN_E_DOMAIN, "record %u (0-based) has a sequence byte of 0x80 or more: the reference indexes its table with a signed char there",
                    u->h_info[kTbBad]);
    }
    u->out_total = res->out_bytes = total;
    u->finished = true;
    return HPN_OK;
}

int hpn_twobit_pack_write(hpn_ctx *c, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_twobit_state *u = c->tb;
    if (!u || !u->finished) return fail(c, HPN_E_STATE, "hpn_twobit_pack_finish first");
    HPN_HIP(c, hipSetDevice(c->device));
    *written = 0;
    if (offset > u->out_total) return fail(c, HPN_E_ARG, "offset %llu beyond the output's %llu bytes", (unsigned long long)offset, (unsigned long long)u->out_total);
    const uint64_t n = u->out_total - offset < cap ? u->out_total - offset : cap;
    if (n && !out) return fail(c, HPN_E_ARG, "out is NULL");
    if (n) HPN_HIP(c, hipMemcpyAsync(out, (const uint8_t *)u->out.p + offset, n, hipMemcpyDefault, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    *written = n;
    return HPN_OK;
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
