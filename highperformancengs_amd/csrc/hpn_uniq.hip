// hpn_uniq.hip -- C ABI of duplicate removal (gzfastq_uniq.c): hpn_fastq_uniq_begin / _add / _finish / _write, and
// hpn_sort_pairs_u64 (the radix sort on its own).  Kernels: kernels/fastq_uniq.hip, kernels/radix_sort.hpp,
// the line index of kernels/fastq_text.hip.
//
// The stream's bytes are appended to a device store as they come (the reference keeps every record in memory too), so a
// chunk is framed where it lies: no carry is copied, the next chunk's framing starts at the first unfinished record.
// The grouping stage and dict.c's walk in closed form: hpn_uniq_group.hpp (shared with hpn_uniqq.hip).
#include "hpn_uniq_group.hpp"

using namespace hpn;

namespace {

constexpr size_t kDescBytes = kUniqDescBytes;
typedef UniqDescHost DescHost;
typedef RecordStore Mate;

void drop_session(hpn_uniq_state *u) { uniq_drop_session(u); }
int fetch_info(hpn_ctx *c, hpn_uniq_state *u) { return uniq_fetch_info(c, u); }
int sort_pairs(hpn_ctx *c, hpn_uniq_state *u, uint64_t *keys, uint32_t *vals, uint32_t n, int begin_bit, int end_bit)
{
    return uniq_sort(c, u, keys, vals, n, begin_bit, end_bit);
}

int session(hpn_ctx *c, hpn_uniq_state **out)
{
    if (!c->uq) c->uq = new hpn_uniq_state;
    hpn_uniq_state *u = c->uq;
    const int rc = uniq_info_alloc(c, u);
    if (rc != HPN_OK) return rc;
    *out = u;
    return HPN_OK;
}


// the whole text of one output on the device (u->out, u->out_total bytes)
int build_output(hpn_ctx *c, hpn_uniq_state *u, int which, int mate)
{
    int rc;
    const uint32_t U = u->U;
    const uint32_t *list = (const uint32_t *)(which == HPN_UNIQ_KEY_ORDER ? u->list_key.p : u->list_table.p);
    if ((rc = need(c, u->size, (size_t)U * 4)) != HPN_OK || (rc = need(c, u->off, ((size_t)U + 1) * 8)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(U) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, launch_uniq_sizes(u->m[mate].desc.p, list, (const uint32_t *)u->rep.p, (const uint32_t *)u->count.p, U, (uint32_t *)u->size.p, c->stream));
    HPN_HIP(c, uniq_scan64((const uint32_t *)u->size.p, (uint64_t *)u->off.p, U, (u64 *)u->status.p, u->d_info + kUiTicket, u->d_info + kUiErr, c->stream));
    uint64_t total = 0;
    HPN_HIP(c, hipMemcpyAsync(&total, (const uint64_t *)u->off.p + U, 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = fetch_info(c, u)) != HPN_OK) return rc;
    u->cached_which = u->cached_mate = -1;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_uniq_write((const uint8_t *)u->m[mate].store.p + kStorePad, u->m[mate].desc.p, list, (const uint32_t *)u->rep.p,
                                 (const uint32_t *)u->count.p, (const uint64_t *)u->off.p, U, (uint8_t *)u->out.p, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    u->out_total = total;
    u->cached_which = which, u->cached_mate = mate;
    return HPN_OK;
}

}  // namespace

namespace hpn {
void uniq_release(hpn_ctx *c)
{
    if (!c->uq) return;
    drop_session(c->uq);
    uniq_info_free(c->uq);
    delete c->uq;
    c->uq = nullptr;
}
}  // namespace hpn

extern "C" {

int hpn_fastq_uniq_begin(hpn_ctx *c, int paired, uint64_t max_bytes, uint32_t hash_bits)
{
    if (!c) return HPN_E_ARG;
    if (hash_bits > 63) return fail(c, HPN_E_ARG, "hash_bits %u (0 = all 64, or 1 .. 63)", hash_bits);
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniq_state *u;
    int rc = session(c, &u);
    if (rc != HPN_OK) return rc;
    drop_session(u);
    if (!max_bytes) {   // half of what is free: the other half is the reserve for the store's growth and the sorts' arrays
        size_t fr = 0, total = 0;
        HPN_HIP(c, hipMemGetInfo(&fr, &total));
        max_bytes = fr / 2;
    }
    u->paired = paired ? 1 : 0, u->limit = max_bytes, u->hash_bits = hash_bits;
    u->open = true;
    return HPN_OK;
}

int hpn_fastq_uniq_add(hpn_ctx *c, int mate, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_uniq_state *u = c->uq;
    if (!u || !u->open || u->finished) return fail(c, HPN_E_STATE, "hpn_fastq_uniq_begin first (or the session was closed by an irregular chunk)");
    if (mate < 0 || mate > u->paired) return fail(c, HPN_E_ARG, "mate %d of a %s session", mate, u->paired ? "paired" : "single-end");
    if (nbytes && !text) return fail(c, HPN_E_ARG, "text is NULL");
    Mate &m = u->m[mate];
    if (m.closed) return fail(c, HPN_E_STATE, "mate %d has had its last chunk", mate);
    HPN_HIP(c, hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    const uint64_t span = m.len - m.pos + nbytes;
    if (span >= (1ull << 31) - 4096) return fail(c, HPN_E_ARG, "chunk of %llu bytes (limit 2^31 - 4 KiB with the unfinished record)", (unsigned long long)nbytes);
    const uint64_t stored = u->m[0].len + u->m[1].len + nbytes;
    if (stored > u->limit) {
        u->open = false;
        return fail(c, HPN_E_CAPACITY, "the store needs %llu bytes, max_bytes is %llu", (unsigned long long)stored, (unsigned long long)u->limit);
    }
    bool close = false;
    const int rc = store_add(c, m, kDescBytes, launch_uniq_keys, text, nbytes, last, &info->n_records, &info->irregular, &close);
    info->store_bytes = u->m[0].len + u->m[1].len;
    if (close) u->open = false;
    return rc;
}

int hpn_fastq_uniq_finish(hpn_ctx *c, hpn_uniq_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_uniq_state *u = c->uq;
    if (!u || !u->open || u->finished) return fail(c, HPN_E_STATE, "no open hpn_fastq_uniq session");
    if (!u->m[0].closed || (u->paired && !u->m[1].closed)) return fail(c, HPN_E_STATE, "every mate needs its last chunk first");
    HPN_HIP(c, hipSetDevice(c->device));
    memset(res, 0, sizeof *res);
    res->unmatched = -1;
    int rc;
    const int paired = u->paired;
    for (int k = 0; k <= paired; ++k)   // (a mate without a byte has no buffers yet)
        if ((rc = grow_keep(c, u->m[k].store, 2 * kStorePad, 0)) != HPN_OK || (rc = grow_keep(c, u->m[k].desc, kDescBytes, 0)) != HPN_OK) return rc;
    const uint8_t *t0 = (const uint8_t *)u->m[0].store.p + kStorePad, *t1 = paired ? (const uint8_t *)u->m[1].store.p + kStorePad : nullptr;
    const void *d0 = u->m[0].desc.p, *d1 = paired ? u->m[1].desc.p : nullptr;
    HPN_HIP(c, hipMemsetAsync(u->d_info, 0, kUiWords * sizeof(uint32_t), c->stream));
    uint32_t N = (uint32_t)u->m[0].n;
    if (paired) {
        const uint32_t n2 = (uint32_t)u->m[1].n, both = N < n2 ? N : n2;
        HPN_HIP(c, hipMemsetAsync(u->d_info + kUiFirstBad, 0xff, sizeof(uint32_t), c->stream));
        HPN_HIP(c, launch_uniq_names(t0, d0, t1, d1, both, u->d_info + kUiFirstBad, c->stream));
        if ((rc = fetch_info(c, u)) != HPN_OK) return rc;
        if (u->h_info[kUiFirstBad] != 0xffffffffu) N = u->h_info[kUiFirstBad], res->unmatched = N;
        else if (N > n2) N = n2, res->unmatched = n2;   // the mate is missing
        if (res->unmatched >= 0) {
            DescHost d;
            HPN_HIP(c, hipMemcpy(&d, (const uint8_t *)d0 + (size_t)N * kDescBytes, kDescBytes, hipMemcpyDeviceToHost));
            HPN_HIP(c, hipMemcpy(res->unmatched_name, t0 + d.off, d.nlen, hipMemcpyDeviceToHost));
            res->unmatched_name[d.nlen] = 0;
        }
    }
    u->N = N;
    res->n_records = N;
    if ((rc = uniq_group(c, u, true, &res->hash_size, &res->hash_clashes)) != HPN_OK) return rc;
    res->n_unique = u->U;
    u->finished = true;
    for (int k = paired; k >= 0; --k) {   // (mate 0 last: its table-order text stays built for the first hpn_fastq_uniq_write)
        if ((rc = build_output(c, u, HPN_UNIQ_TABLE_ORDER, k)) != HPN_OK) return rc;
        res->out_bytes[k] = u->out_total;
    }
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    return HPN_OK;
}

int hpn_fastq_uniq_write(hpn_ctx *c, int which, int mate, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_uniq_state *u = c->uq;
    if (!u || !u->finished) return fail(c, HPN_E_STATE, "hpn_fastq_uniq_finish first");
    if (which != HPN_UNIQ_TABLE_ORDER && which != HPN_UNIQ_KEY_ORDER) return fail(c, HPN_E_ARG, "unknown output %d", which);
    if (mate < 0 || mate > u->paired || (u->paired && which == HPN_UNIQ_KEY_ORDER))
        return fail(c, HPN_E_ARG, "output %d of mate %d: a paired session has the table order of mates 0 and 1, a single-end one both orders of mate 0", which, mate);
    HPN_HIP(c, hipSetDevice(c->device));
    *written = 0;
    int rc;
    if ((u->cached_which != which || u->cached_mate != mate) && (rc = build_output(c, u, which, mate)) != HPN_OK) return rc;
    if (offset > u->out_total) return fail(c, HPN_E_ARG, "offset %llu beyond the output's %llu bytes", (unsigned long long)offset, (unsigned long long)u->out_total);
    const uint64_t n = u->out_total - offset < cap ? u->out_total - offset : cap;
    if (n && !out) return fail(c, HPN_E_ARG, "out is NULL");
    if (n) HPN_HIP(c, hipMemcpyAsync(out, (const uint8_t *)u->out.p + offset, n, hipMemcpyDefault, c->stream));
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    *written = n;
    return HPN_OK;
}

int hpn_sort_pairs_u64(hpn_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n)
{
    if (!c || (n && (!keys || !vals))) return HPN_E_ARG;
    if (n >= (1ull << 31)) return fail(c, HPN_E_DOMAIN, "2^31 or more keys");
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniq_state *u;
    int rc = session(c, &u);
    if (rc != HPN_OK) return rc;
    if (u->open && !u->finished) return fail(c, HPN_E_STATE, "a hpn_fastq_uniq session is collecting text: its work space is in use");
    struct Pair {   // the caller's arrays on the device, for this call only
        Scratch k, v;
        ~Pair()
        {
            release_scratch(k);
            release_scratch(v);
        }
    } d;
    if ((rc = need(c, d.k, (size_t)n * 8)) != HPN_OK || (rc = need(c, d.v, (size_t)n * 4)) != HPN_OK) return rc;
    HPN_HIP(c, hipMemsetAsync(u->d_info, 0, kUiWords * sizeof(uint32_t), c->stream));
    if (n) {
        HPN_HIP(c, hipMemcpyAsync(d.k.p, keys, (size_t)n * 8, hipMemcpyDefault, c->stream));
        HPN_HIP(c, hipMemcpyAsync(d.v.p, vals, (size_t)n * 4, hipMemcpyDefault, c->stream));
    }
    if ((rc = sort_pairs(c, u, (uint64_t *)d.k.p, (uint32_t *)d.v.p, (uint32_t)n, 0, 64)) != HPN_OK) return rc;
    if (n) {
        HPN_HIP(c, hipMemcpyAsync(keys, d.k.p, (size_t)n * 8, hipMemcpyDefault, c->stream));
        HPN_HIP(c, hipMemcpyAsync(vals, d.v.p, (size_t)n * 4, hipMemcpyDefault, c->stream));
    }
    return fetch_info(c, u);   // (waits for the stream: the arrays are free to go)
}

}  // extern "C"
