// hpn_store.hpp -- the device store behind the nine store-backed entry points (hpn_fastq_uniq_*, _uniqq_*, _usort_*, _sort_*, _pair_*,
// hpn_twobit_pack_*, hpn_mrle_*, hpn_rfastqc_*, hpn_kseq_*) and the session around it.  The store: a stream's bytes are appended as they come and framed WHERE THEY
// LIE (no carry is copied: the next chunk's framing starts at the first unfinished record), one descriptor per record.  What a
// descriptor holds is the caller's: it hands in the hook that writes them (frame_by<> over kernels/fastq_uniq.hip: k_uniq_keys
// or kernels/fastq_sort.hip: k_sort_frame; hpn_kseq.hip: kseq_frame) behind the line index of kernels/fastq_text.hip.  The
// session: one or two stores under one byte limit, the _begin / _add / _finish / _write life cycle and its messages, and the
// info block the scans report through.  Every buffer here owns what it holds (Scratch, InfoBlock): a state that goes frees them,
// and a family drops a session by assigning a fresh value to what a new session must not inherit.
#pragma once
#include <string.h>

#include <utility>

#include "hpn_ctx.hpp"

namespace hpn {
// kernels/fastq_text.hip
hipError_t launch_text_lines(const uint8_t *d_slot, uint32_t begin, uint32_t end, int last, uint32_t own_end, uint32_t *d_nl,
                             uint32_t nl_cap, u64 *d_status, uint32_t *d_state, hipStream_t st);
uint64_t text_tiles1(uint32_t begin, uint32_t end);
uint64_t text_tiles2(uint32_t nl_cap);
// kernels/fastq_sort.hip: the framing behind kernels/sort_desc.hpp
hipError_t launch_sort_frame(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                             void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *user);
// kernels/fastq_uniq.hip: the scans and the radix sort (radix_sort.hpp)
hipError_t uniq_scan32(const uint32_t *d_in, uint32_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st);
hipError_t uniq_scan64(const uint32_t *d_in, uint64_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st);
hipError_t uniq_scan64w(const uint64_t *d_in, uint64_t *d_out, uint64_t n, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t st);
uint64_t uniq_scan_tiles(uint64_t n);
uint64_t uniq_sort_hist_words(uint32_t n);
hipError_t uniq_sort_pairs(uint64_t *d_keys, uint32_t *d_vals, uint32_t n, int begin_bit, int end_bit, uint64_t *d_keys_tmp,
                           uint32_t *d_vals_tmp, uint32_t *d_hist, uint32_t *d_offs, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err,
                           hipStream_t st);
hipError_t uniq_sort_pairs_digits(uint64_t *d_keys, uint32_t *d_vals, uint32_t n, uint32_t digits, uint64_t *d_keys_tmp, uint32_t *d_vals_tmp,
                                  uint32_t *d_hist, uint32_t *d_offs, u64 *d_status, uint32_t *d_ticket, uint32_t *d_err, hipStream_t s);

constexpr uint32_t kStorePad = 64;    // bytes in front of the stream's first byte and behind its last (the kernels' 16-byte loads)
constexpr int kStateWords = 16;       // kernels/text_common.hpp: kTs*
enum { kTsLines = 0, kTsRecs, kTsFlags, kTsUnterminated, kTsConsumed, kTsErr = 7 };

struct RecordStore {
    Scratch store, desc;
    uint64_t len = 0, pos = 0, n = 0;   // stream bytes stored; where the first unframed record starts; records framed
    bool closed = false;
};

// The frame hook: writes the descriptors of the records that the line index d_nl holds (run over an upper bound of records) on
// the context's stream, and returns an HPN status with its message set; a hook that fails closes the session.  `user` is the
// caller's own (the kernels of the gzgets families take none: nullptr).
struct FrameArgs {
    const uint8_t *d_slot;
    const uint32_t *d_nl;
    uint32_t begin, end;
    int last;
    uint64_t origin;
    void *d_desc;
    uint32_t max_records;
    uint32_t *d_state;
    void *user;
};
typedef int (*store_frame_fn)(hpn_ctx *c, const FrameArgs &a);

// the hook over a plain launcher (launch_sort_frame, launch_uniq_keys, launch_uniqq_keys)
typedef hipError_t (*frame_launch_fn)(const uint8_t *d_slot, const uint32_t *d_nl, uint32_t begin, uint32_t end, int last, uint64_t origin,
                                      void *d_desc, uint32_t max_records, uint32_t *d_state, hipStream_t st, void *user);
template <frame_launch_fn launch>
int frame_by(hpn_ctx *c, const FrameArgs &a)
{
    HPN_HIP(c, launch(a.d_slot, a.d_nl, a.begin, a.end, a.last, a.origin, a.d_desc, a.max_records, a.d_state, c->stream, a.user));
    return HPN_OK;
}

// a buffer that keeps its first `keep` bytes when it grows (doubling: the copies add up to less than one more pass)
inline int grow_keep(hpn_ctx *c, Scratch &s, size_t bytes, size_t keep)
{
    if (bytes <= s.cap) return HPN_OK;
    size_t want = s.cap * 2 > bytes ? s.cap * 2 : bytes;
    if (want < ((size_t)1 << 20)) want = (size_t)1 << 20;
    Scratch grown;   // (a copy that fails frees it and leaves `s` as it was)
    hipError_t e = hipMalloc(&grown.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        grown.p = nullptr;
        return fail(c, HPN_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    grown.cap = want;
    if (s.p) {
        if (keep) HPN_HIP(c, hipMemcpyAsync(grown.p, s.p, keep, hipMemcpyDeviceToDevice, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
    }
    s = std::move(grown);
    return HPN_OK;
}

inline int need(hpn_ctx *c, Scratch &s, size_t bytes) { return scratch_reserve(c, s, bytes + 64); }

// One chunk into the store (the caller has checked the chunk's size and the store's limit).  *n_records: records framed by this
// call; *irregular: HPN_TEXT_* reasons (nothing of the chunk counts then); *close: the session cannot go on (irregular text, an
// error of the device, 2^31 records) -- the status is the call's.  record_lines: the fewest lines a record takes -- the bound
// the descriptors are sized and `frame` is launched by is the chunk's lines / record_lines (4 for four gzgets per record, 1 for
// kseq framing, where a FASTA header alone is a record).
inline int store_add(hpn_ctx *c, RecordStore &m, size_t desc_bytes, store_frame_fn frame, void *user, uint32_t record_lines, const void *text, uint64_t nbytes, int last,
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
    const uint32_t max_records = h[kTsLines] / record_lines;
    if (m.n + max_records >= (1ull << 31)) {
        *close = true;
        return fail(c, HPN_E_DOMAIN, "2^31 or more records");
    }
    if ((rc = grow_keep(c, m.desc, (size_t)(m.n + max_records + 1) * desc_bytes, (size_t)m.n * desc_bytes)) != HPN_OK) return rc;
    const FrameArgs fa = {slot, (const uint32_t *)c->t_nl.p, begin, end, last, m.pos, (uint8_t *)m.desc.p + (size_t)m.n * desc_bytes, max_records,
                          c->t_state, user};
    if ((rc = frame(c, fa)) != HPN_OK) {   // the chunk is stored but not framed
        *close = true;
        return rc;
    }
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

// ---- the session ----  (`api`: the family's name in messages -- "hpn_fastq_sort", ... -- from the caller: there is no state before
// the first _begin)

// The device's info block (uint32 words): the scans' and sorts' hand-off ticket and error flag, then the family's own words.
enum { kInfoTicket = 0, kInfoErr = 1, kInfoOwn = 2, kInfoWords = 16 };

struct InfoBlock {
    uint32_t *d = nullptr, *h = nullptr;   // kInfoWords each; h: the pinned mirror
    InfoBlock() = default;
    InfoBlock(InfoBlock &&o) noexcept : d(o.d), h(o.h) { o.d = o.h = nullptr; }
    InfoBlock &operator=(InfoBlock &&o) noexcept
    {
        if (this != &o) {
            release();
            d = o.d, h = o.h;
            o.d = o.h = nullptr;
        }
        return *this;
    }
    ~InfoBlock() { release(); }
    void release()
    {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
    }
    uint32_t *ticket() const { return d + kInfoTicket; }
    uint32_t *err() const { return d + kInfoErr; }
    int alloc(hpn_ctx *c)   // on first use
    {
        if (!d) HPN_HIP(c, hipMalloc((void **)&d, kInfoWords * sizeof(uint32_t)));
        if (!h) HPN_HIP(c, hipHostMalloc((void **)&h, kInfoWords * sizeof(uint32_t), hipHostMallocDefault));
        return HPN_OK;
    }
    int zero(hpn_ctx *c)
    {
        HPN_HIP(c, hipMemsetAsync(d, 0, kInfoWords * sizeof(uint32_t), c->stream));
        return HPN_OK;
    }
    int fetch(hpn_ctx *c)   // the block on the host; waits for the stream
    {
        HPN_HIP(c, hipMemcpyAsync(h, d, kInfoWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        if (h[kInfoErr]) return fail(c, HPN_E_HIP, "prefix-scan hand-off timed out");
        return HPN_OK;
    }
};

struct StoreSession {
    int n_streams = 1;
    RecordStore m[2];
    uint64_t limit = 0;
    bool open = false, finished = false;
    InfoBlock info;
    const uint8_t *text(int k) const { return (const uint8_t *)m[k].store.p + kStorePad; }
};

// the stores go, the info block stays
inline void session_drop(StoreSession &s)
{
    for (RecordStore &m : s.m) m = RecordStore();
    s.open = s.finished = false;
}

// _begin, behind the family's own drop: the info block on first use, the limit, open
inline int session_begin(hpn_ctx *c, StoreSession &s, int n_streams, uint64_t max_bytes)
{
    const int rc = s.info.alloc(c);
    if (rc != HPN_OK) return rc;
    session_drop(s);
    if (!max_bytes) {   // half of what is free: the other half is the reserve for the store's growth, the sorts' arrays and the output
        size_t fr = 0, total = 0;
        HPN_HIP(c, hipMemGetInfo(&fr, &total));
        max_bytes = fr / 2;
    }
    s.n_streams = n_streams, s.limit = max_bytes;
    s.open = true;
    return HPN_OK;
}

// _add (Info: hpn_uniq_info / hpn_sort_info).  The limit counts every stream; info->store_bytes is every stream's bytes, or with
// own_bytes the fed stream's.  A chunk beyond the limit and an irregular chunk close the session; NULL text and a span beyond
// 2^31 - 4 KiB do not.
template <class Info>
int session_add(hpn_ctx *c, StoreSession *s, const char *api, int mate, size_t desc_bytes, store_frame_fn frame, void *user, uint32_t record_lines,
                const void *text,
                uint64_t nbytes, int last, bool own_bytes, Info *info)
{
    if (!s || !s->open || s->finished) return fail(c, HPN_E_STATE, "%s_begin first (or the session was closed by an irregular chunk)", api);
    if (mate < 0 || mate >= s->n_streams) return fail(c, HPN_E_ARG, "mate %d of a %s session", mate, s->n_streams > 1 ? "paired" : "single-end");
    if (nbytes && !text) return fail(c, HPN_E_ARG, "text is NULL");
    RecordStore &m = s->m[mate];
    if (m.closed) return s->n_streams > 1 ? fail(c, HPN_E_STATE, "mate %d has had its last chunk", mate) : fail(c, HPN_E_STATE, "the stream has had its last chunk");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t span = m.len - m.pos + nbytes;
    if (span >= (1ull << 31) - 4096) return fail(c, HPN_E_ARG, "chunk of %llu bytes (limit 2^31 - 4 KiB with the unfinished record)", (unsigned long long)nbytes);
    const uint64_t stored = s->m[0].len + s->m[1].len + nbytes;
    if (stored > s->limit) {
        s->open = false;
        return fail(c, HPN_E_CAPACITY, "the store needs %llu bytes, max_bytes is %llu", (unsigned long long)stored, (unsigned long long)s->limit);
    }
    bool close = false;
    const int rc = store_add(c, m, desc_bytes, frame, user, record_lines, text, nbytes, last, &info->n_records, &info->irregular, &close);
    info->store_bytes = own_bytes ? m.len : s->m[0].len + s->m[1].len;
    if (close) s->open = false;
    return rc;
}

// What every _finish opens with: the session is open, every stream has had its last chunk; a stream without a byte gets its
// (smallest) buffers, the info block is zeroed.
inline int session_finish_begin(hpn_ctx *c, StoreSession *s, const char *api, size_t desc_bytes)
{
    if (!s || !s->open || s->finished) return fail(c, HPN_E_STATE, "no open %s session", api);
    for (int k = 0; k < s->n_streams; ++k)
        if (!s->m[k].closed) return fail(c, HPN_E_STATE, s->n_streams > 1 ? "every mate needs its last chunk first" : "the stream needs its last chunk first");
    HPN_HIP(c, hipSetDevice(c->device));
    int rc;
    for (int k = 0; k < s->n_streams; ++k)
        if ((rc = grow_keep(c, s->m[k].store, 2 * kStorePad, 0)) != HPN_OK || (rc = grow_keep(c, s->m[k].desc, desc_bytes, 0)) != HPN_OK) return rc;
    return s->info.zero(c);
}

// n 32-bit sizes -> n + 1 64-bit offsets; *total: the last one, on the host
inline int scan_sizes(hpn_ctx *c, InfoBlock &info, Scratch &status, const Scratch &size, const Scratch &off, uint64_t n, uint64_t *total)
{
    int rc;
    if ((rc = need(c, status, uniq_scan_tiles(n) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, uniq_scan64((const uint32_t *)size.p, (uint64_t *)off.p, n, (u64 *)status.p, info.ticket(), info.err(), c->stream));
    HPN_HIP(c, hipMemcpyAsync(total, (const uint64_t *)off.p + n, 8, hipMemcpyDeviceToHost, c->stream));
    return info.fetch(c);
}

// What every _write opens with, and its slice copy: up to `cap` bytes of the `total` that lie in `out`, from `offset` on
inline int session_write_begin(hpn_ctx *c, const StoreSession *s, const char *api, uint64_t *written)
{
    if (!s || !s->finished) return fail(c, HPN_E_STATE, "%s_finish first", api);
    HPN_HIP(c, hipSetDevice(c->device));
    *written = 0;
    return HPN_OK;
}

inline int session_write_slice(hpn_ctx *c, const Scratch &out, uint64_t total, uint64_t offset, void *dst, uint64_t cap, uint64_t *written)
{
    if (offset > total) return fail(c, HPN_E_ARG, "offset %llu beyond the output's %llu bytes", (unsigned long long)offset, (unsigned long long)total);
    const uint64_t n = total - offset < cap ? total - offset : cap;
    if (n && !dst) return fail(c, HPN_E_ARG, "out is NULL");
    if (n) HPN_HIP(c, hipMemcpyAsync(dst, (const uint8_t *)out.p + offset, n, hipMemcpyDefault, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    *written = n;
    return HPN_OK;
}

}  // namespace hpn
