// hpn_uniq.hip -- C ABI of duplicate removal (gzfastq_uniq.c): hpn_fastq_uniq_begin / _add / _finish / _write, and
// hpn_sort_pairs_u64 / _bits / _digits and hpn_excl_scan (the radix sort and the prefix scan on their own).  Kernels: kernels/fastq_uniq.hip, kernels/radix_sort.hpp,
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

// The state the primitives' own entry points run in: the uniq family's work space, which a collecting session has in use.
int prim_state(hpn_ctx *c, hpn_uniq_state **out)
{
    hpn_uniq_state *u = state_make<hpn_uniq_state>(c);
    const int rc = u->s.info.alloc(c);
    if (rc != HPN_OK) return rc;
    if (u->s.open && !u->s.finished) return fail(c, HPN_E_STATE, "a hpn_fastq_uniq session is collecting text: its work space is in use");
    *out = u;
    return HPN_OK;
}

// hpn_sort_pairs_u64_*: the caller's n pairs onto the device, sort(u, keys, vals) over them there, and back
template <typename Sort>
int sort_pairs_call(hpn_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n, Sort sort)
{
    if (n && (!keys || !vals)) return HPN_E_ARG;
    if (n >= (1ull << 31)) return fail(c, HPN_E_DOMAIN, "2^31 or more keys");
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniq_state *u = nullptr;
    int rc = prim_state(c, &u);
    if (rc != HPN_OK) return rc;
    Scratch k, v;   // the caller's arrays on the device, for this call only
    if ((rc = need(c, k, (size_t)n * 8)) != HPN_OK || (rc = need(c, v, (size_t)n * 4)) != HPN_OK || (rc = u->s.info.zero(c)) != HPN_OK) return rc;
    if (n) {
        HPN_HIP(c, hipMemcpyAsync(k.p, keys, (size_t)n * 8, hipMemcpyDefault, c->stream));
        HPN_HIP(c, hipMemcpyAsync(v.p, vals, (size_t)n * 4, hipMemcpyDefault, c->stream));
    }
    if ((rc = sort(u, (uint64_t *)k.p, (uint32_t *)v.p)) != HPN_OK) return rc;
    if (n) {
        HPN_HIP(c, hipMemcpyAsync(keys, k.p, (size_t)n * 8, hipMemcpyDefault, c->stream));
        HPN_HIP(c, hipMemcpyAsync(vals, v.p, (size_t)n * 4, hipMemcpyDefault, c->stream));
    }
    return u->s.info.fetch(c);   // (waits for the stream: the arrays are free to go)
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

int hpn_sort_pairs_u64(hpn_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n) { return hpn_sort_pairs_u64_bits(c, keys, vals, n, 0, 64); }

int hpn_sort_pairs_u64_bits(hpn_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n, int begin_bit, int end_bit)
{
    if (!c) return HPN_E_ARG;
    if (begin_bit < 0 || begin_bit > end_bit || end_bit > 64) return fail(c, HPN_E_ARG, "key bits [%d, %d): 0 <= begin <= end <= 64", begin_bit, end_bit);
    return sort_pairs_call(c, keys, vals, n, [&](hpn_uniq_state *u, uint64_t *k, uint32_t *v) { return uniq_sort(c, u, k, v, (uint32_t)n, begin_bit, end_bit); });
}

int hpn_sort_pairs_u64_digits(hpn_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n, uint32_t digits)
{
    if (!c) return HPN_E_ARG;
    if (digits > 255u) return fail(c, HPN_E_ARG, "digit mask %u: a key has 8 bytes", digits);
    return sort_pairs_call(c, keys, vals, n, [&](hpn_uniq_state *u, uint64_t *k, uint32_t *v) {
        int rc;
        if ((rc = uniq_sort_space(c, u, (uint32_t)n)) != HPN_OK) return rc;
        HPN_HIP(c, uniq_sort_pairs_digits(k, v, (uint32_t)n, digits, (uint64_t *)u->key_tmp.p, (uint32_t *)u->val_tmp.p, (uint32_t *)u->hist.p,
                                          (uint32_t *)u->offs.p, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
        return (int)HPN_OK;
    });
}

int hpn_excl_scan(hpn_ctx *c, const void *in, int in_bits, void *out, int out_bits, uint64_t n)
{
    if (!c || !out || (n && !in)) return HPN_E_ARG;
    if (!((in_bits == 32 && (out_bits == 32 || out_bits == 64)) || (in_bits == 64 && out_bits == 64)))
        return fail(c, HPN_E_ARG, "scan of %d-bit items into %d-bit sums: 32 -> 32, 32 -> 64 or 64 -> 64", in_bits, out_bits);
    if (n >= (1ull << 31)) return fail(c, HPN_E_DOMAIN, "2^31 or more items");
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_uniq_state *u = nullptr;
    int rc = prim_state(c, &u);
    if (rc != HPN_OK) return rc;
    const size_t ib = (size_t)in_bits / 8, ob = (size_t)out_bits / 8;
    Scratch a, b;   // the caller's arrays on the device, for this call only
    if ((rc = need(c, a, (size_t)n * ib)) != HPN_OK || (rc = need(c, b, ((size_t)n + 1) * ob)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(n) * 8)) != HPN_OK || (rc = u->s.info.zero(c)) != HPN_OK)
        return rc;
    if (n) HPN_HIP(c, hipMemcpyAsync(a.p, in, (size_t)n * ib, hipMemcpyDefault, c->stream));
    u64 *status = (u64 *)u->status.p;
    uint32_t *ticket = u->s.info.ticket(), *err = u->s.info.err();
    if (in_bits == 64) HPN_HIP(c, uniq_scan64w((const uint64_t *)a.p, (uint64_t *)b.p, n, status, ticket, err, c->stream));
    else if (out_bits == 64) HPN_HIP(c, uniq_scan64((const uint32_t *)a.p, (uint64_t *)b.p, n, status, ticket, err, c->stream));
    else HPN_HIP(c, uniq_scan32((const uint32_t *)a.p, (uint32_t *)b.p, n, status, ticket, err, c->stream));
    HPN_HIP(c, hipMemcpyAsync(out, b.p, ((size_t)n + 1) * ob, hipMemcpyDefault, c->stream));
    return u->s.info.fetch(c);   // (waits for the stream: the arrays are free to go)
}

}  // extern "C"
