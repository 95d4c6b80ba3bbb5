// hpn_store.hpp -- the device store behind hpn_fastq_uniq_* and hpn_fastq_sort_*: a stream's bytes are appended as they come and
// framed WHERE THEY LIE (no carry is copied: the next chunk's framing starts at the first unfinished record), one descriptor per
// record.  What a descriptor holds is the caller's: it hands in the kernel that writes them (kernels/fastq_uniq.hip: k_uniq_keys,
// kernels/fastq_sort.hip: k_sort_frame) behind the line index of kernels/fastq_text.hip.
#pragma once
#include "hpn_ctx.hpp"

namespace hpn {
// kernels/fastq_text.hip
hipError_t launch_text_lines(const uint8_t *d_slot, uint32_t begin, uint32_t end, int last, uint32_t own_end, uint32_t *d_nl,
                             uint32_t nl_cap, u64 *d_status, uint32_t *d_state, hipStream_t st);
uint64_t text_tiles1(uint32_t begin, uint32_t end);
uint64_t text_tiles2(uint32_t nl_cap);

constexpr uint32_t kStorePad = 64;    // bytes in front of the stream's first byte and behind its last (the kernels' 16-byte loads)
constexpr int kStateWords = 16;       // kernels/text_common.hpp: kTs*
enum { kTsLines = 0, kTsRecs, kTsFlags, kTsUnterminated, kTsConsumed, kTsErr = 7 };

struct RecordStore {
    Scratch store, desc;
    uint64_t len = 0, pos = 0, n = 0;   // stream bytes stored; where the first unframed record starts; records framed
    bool closed = false;
};

// writes the descriptors of the records that the line index d_nl holds (launched over an upper bound of records)
typedef hipError_t (*store_frame_fn)(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                                     void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st);

inline void release_scratch(Scratch &s)
{
    if (s.p) (void)hipFree(s.p);
    s.p = nullptr, s.cap = 0;
}

inline void store_release(RecordStore &m)
{
    release_scratch(m.store);
    release_scratch(m.desc);
    m.len = m.pos = m.n = 0, m.closed = false;
}

// a buffer that keeps its first `keep` bytes when it grows (doubling: the copies add up to less than one more pass)
inline int grow_keep(hpn_ctx *c, Scratch &s, size_t bytes, size_t keep)
{
    if (bytes <= s.cap) return HPN_OK;
    size_t want = s.cap * 2 > bytes ? s.cap * 2 : bytes;
    if (want < ((size_t)1 << 20)) want = (size_t)1 << 20;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, HPN_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    if (s.p) {
        if (keep) HPN_HIP(c, hipMemcpyAsync(p, s.p, keep, hipMemcpyDeviceToDevice, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        HPN_HIP(c, hipFree(s.p));
    }
    s.p = p, s.cap = want;
    return HPN_OK;
}

inline int need(hpn_ctx *c, Scratch &s, size_t bytes) { return scratch_reserve(c, s, bytes + 64); }

// One chunk into the store (the caller has checked the chunk's size and the store's limit).  *n_records: records framed by this
// call; *irregular: HPN_TEXT_* reasons (nothing of the chunk counts then); *close: the session cannot go on (irregular text, an
// error of the device, 2^31 records) -- the status is the call's.
inline int store_add(hpn_ctx *c, RecordStore &m, size_t desc_bytes, store_frame_fn frame, const void *text, uint64_t nbytes, int last,
                     uint64_t *n_records, uint32_t *irregular, bool *close)
{
    *n_records = 0, *irregular = 0, *close = false;
    const uint64_t span = m.len - m.pos + nbytes;
    int rc;
    if (!c->t_state) {
        HPN_HIP(c, hipMalloc((void **)&c->t_state, kStateWords * sizeof(uint32_t)));
        HPN_HIP(c, hipHostMalloc((void **)&c->h_tstate, kStateWords * sizeof(uint32_t), hipHostMallocDefault));
    }
    if ((rc = grow_keep(c, m.store, (size_t)kStorePad + m.len + nbytes + kStorePad, (size_t)kStorePad + m.len)) != HPN_OK) return rc;
    uint8_t *store = (uint8_t *)m.store.p;
    if (nbytes) HPN_HIP(c, hipMemcpyAsync(store + kStorePad + m.len, text, nbytes, hipMemcpyDefault, c->stream));
    m.len += nbytes;
    if (last) m.closed = true;
    if (span == 0) {
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        return HPN_OK;
    }
    // stream byte s lies at store[kStorePad + s]; the framing kernels want a 16-byte aligned base
    const uint64_t slot_off = m.pos & ~15ull;
    const uint8_t *slot = store + slot_off;
    const uint32_t begin = kStorePad + (uint32_t)(m.pos - slot_off), end = begin + (uint32_t)span;
    // one line per 4 bytes is what the index is sized for; text denser than that is indexed again with room for a line per byte
    const uint32_t *h = c->h_tstate;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamText], c->stream));
    for (int attempt = 0;; ++attempt) {
        const uint32_t nl_cap = attempt ? (end - begin + 20u) & ~3u : (((end - begin) / 4u) + 16u) & ~3u;
        if ((rc = scratch_reserve(c, c->t_nl, (size_t)nl_cap * sizeof(uint32_t) + 64)) != HPN_OK) return rc;
        if ((rc = scratch_reserve(c, c->t_status, (text_tiles1(begin, end) + text_tiles2(nl_cap)) * sizeof(u64))) != HPN_OK) return rc;
        HPN_HIP(c, launch_text_lines(slot, begin, end, last, 0u, (uint32_t *)c->t_nl.p, nl_cap, (u64 *)c->t_status.p, c->t_state, c->stream));
        HPN_HIP(c, hipMemcpyAsync(c->h_tstate, c->t_state, kStateWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));   // (the text has been copied: the caller's buffer is free)
        if (h[kTsErr]) {
            *close = true;
            return fail(c, HPN_E_HIP, "prefix-scan hand-off timed out");
        }
        if (h[kTsFlags] == HPN_TEXT_DENSE && attempt == 0) continue;
        break;
    }
    if (h[kTsFlags]) {
        *irregular = h[kTsFlags], *close = true;
        return HPN_OK;
    }
    const uint32_t max_records = h[kTsLines] / 4u;
    if (m.n + max_records >= (1ull << 31)) {
        *close = true;
        return fail(c, HPN_E_DOMAIN, "2^31 or more records");
    }
    if ((rc = grow_keep(c, m.desc, (size_t)(m.n + max_records + 1) * desc_bytes, (size_t)m.n * desc_bytes)) != HPN_OK) return rc;
    HPN_HIP(c, frame(slot, (const uint32_t *)c->t_nl.p, begin, end, last, m.pos, (uint8_t *)m.desc.p + (size_t)m.n * desc_bytes, max_records,
                     c->t_state, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamText], c->stream));
    c->ev_valid[kFamText] = true;
    HPN_HIP(c, hipMemcpyAsync(c->h_tstate, c->t_state, kStateWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    if (h[kTsFlags]) {
        *irregular = h[kTsFlags], *close = true;
        return HPN_OK;
    }
    *n_records = h[kTsRecs];
    m.n += h[kTsRecs];
    m.pos += h[kTsConsumed] - begin;
    return HPN_OK;
}

}  // namespace hpn
