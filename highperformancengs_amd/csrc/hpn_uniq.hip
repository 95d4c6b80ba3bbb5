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

// the whole text of one output on the device (u->out, u->out_total bytes)
int build_output(hpn_ctx *c, hpn_uniq_state *u, int which, int mate)
{
    int rc;
    const uint32_t U = u->U;
    const uint32_t *list = (const uint32_t *)(which == HPN_UNIQ_KEY_ORDER ? u->list_key.p : u->list_table.p);
    if ((rc = need(c, u->size, (size_t)U * 4)) != HPN_OK || (rc = need(c, u->off, ((size_t)U + 1) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, launch_uniq_sizes(u->s.m[mate].desc.p, list, (const uint32_t *)u->rep.p, (const uint32_t *)u->count.p, U, (uint32_t *)u->size.p, c->stream));
    uint64_t total = 0;
    if ((rc = scan_sizes(c, u->s.info, u->status, u->size, u->off, U, &total)) != HPN_OK) return rc;
    u->cached_which = u->cached_mate = -1;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_uniq_write((const uint8_t *)u->s.m[mate].store.p + kStorePad, u->s.m[mate].desc.p, list, (const uint32_t *)u->rep.p,
                                 (const uint32_t *)u->count.p, (const uint64_t *)u->off.p, U, (uint8_t *)u->out.p, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    u->out_total = total;
    u->cached_which = which, u->cached_mate = mate;
    return HPN_OK;
}

}  // namespace

extern "C" {

int hpn_fastq_uniq_begin(hpn_ctx *c, int paired, uint64_t max_bytes, uint32_t hash_bits)
{
    if (!c) return HPN_E_ARG;
    if (hash_bits > 63) return fail(c, HPN_E_ARG, "hash_bits %u (0 = all 64, or 1 .. 63)", hash_bits);
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniq_state *u = state_make<hpn_uniq_state>(c);
    uniq_drop_session(u);
    return uniq_begin(c, u, paired, max_bytes, hash_bits);
}

int hpn_fastq_uniq_add(hpn_ctx *c, int mate, const void *text, uint64_t nbytes, int last, hpn_uniq_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_uniq_state *u = state<hpn_uniq_state>(c);
    return session_add(c, u ? &u->s : nullptr, "hpn_fastq_uniq", mate, kUniqDescBytes, frame_by<launch_uniq_keys>, nullptr, 4u, text, nbytes, last, false, info);
}

int hpn_fastq_uniq_finish(hpn_ctx *c, hpn_uniq_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_uniq_state *u = state<hpn_uniq_state>(c);
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_fastq_uniq", kUniqDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    res->unmatched = -1;
    const int paired = u->paired;
    uint32_t N = (uint32_t)u->s.m[0].n;
    if ((rc = uniq_match_mates(c, u, &N, &res->unmatched, res->unmatched_name)) != HPN_OK) return rc;
    u->N = N;
    res->n_records = N;
    if ((rc = uniq_group(c, u, true, &res->hash_size, &res->hash_clashes)) != HPN_OK) return rc;
    res->n_unique = u->U;
    u->s.finished = true;
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
    hpn_uniq_state *u = state<hpn_uniq_state>(c);
    int rc;
    if ((rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_fastq_uniq", written)) != HPN_OK) return rc;
    if (which != HPN_UNIQ_TABLE_ORDER && which != HPN_UNIQ_KEY_ORDER) return fail(c, HPN_E_ARG, "unknown output %d", which);
    if (mate < 0 || mate > u->paired || (u->paired && which == HPN_UNIQ_KEY_ORDER))
        return fail(c, HPN_E_ARG, "output %d of mate %d: a paired session has the table order of mates 0 and 1, a single-end one both orders of mate 0", which, mate);
    if ((u->cached_which != which || u->cached_mate != mate) && (rc = build_output(c, u, which, mate)) != HPN_OK) return rc;
    return session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

int hpn_sort_pairs_u64(hpn_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n)
{
    if (!c || (n && (!keys || !vals))) return HPN_E_ARG;
    if (n >= (1ull << 31)) return fail(c, HPN_E_DOMAIN, "2^31 or more keys");
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniq_state *u = state_make<hpn_uniq_state>(c);
    int rc = u->s.info.alloc(c);
    if (rc != HPN_OK) return rc;
    if (u->s.open && !u->s.finished) return fail(c, HPN_E_STATE, "a hpn_fastq_uniq session is collecting text: its work space is in use");
    Scratch k, v;   // the caller's arrays on the device, for this call only
    if ((rc = need(c, k, (size_t)n * 8)) != HPN_OK || (rc = need(c, v, (size_t)n * 4)) != HPN_OK || (rc = u->s.info.zero(c)) != HPN_OK) return rc;
    if (n) {
        HPN_HIP(c, hipMemcpyAsync(k.p, keys, (size_t)n * 8, hipMemcpyDefault, c->stream));
        HPN_HIP(c, hipMemcpyAsync(v.p, vals, (size_t)n * 4, hipMemcpyDefault, c->stream));
    }
    if ((rc = uniq_sort(c, u, (uint64_t *)k.p, (uint32_t *)v.p, (uint32_t)n, 0, 64)) != HPN_OK) return rc;
    if (n) {
        HPN_HIP(c, hipMemcpyAsync(keys, k.p, (size_t)n * 8, hipMemcpyDefault, c->stream));
        HPN_HIP(c, hipMemcpyAsync(vals, v.p, (size_t)n * 4, hipMemcpyDefault, c->stream));
    }
    return u->s.info.fetch(c);   // (waits for the stream: the arrays are free to go)
}

}  // extern "C"
