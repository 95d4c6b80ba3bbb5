// hpn_sort.hip -- C ABI of the whole-file sort (gzfastq_sort.c): hpn_fastq_sort_begin / _add / _finish / _write.
// Kernels: kernels/fastq_sort.hip, the radix sort and the scans of kernels/fastq_uniq.hip (radix_sort.hpp), the line index of
// kernels/fastq_text.hip.  The store and its framing in place: hpn_store.hpp.
//
// The order is (key line's length, its bytes as unsigned, input ordinal), built most significant bytes first.  Round 0 sorts
// all records by length and the first 6 bytes; round k >= 1 sorts the records of the runs that are still undecided by their
// next 8 bytes and then by run number -- both sorts stable, both over the digits in which two keys differ and no others -- so
// that the i-th sorted element goes to the i-th tied position.  A run whose neighbours are all equal behind the bytes sorted
// so far is settled: duplicates leave after one look, and so does every run whose bytes are used up.
#include "hpn_sorter.hpp"
#include "kernels/sort_desc.hpp"

namespace hpn {
struct SortTied {   // kernels/fastq_sort.hip
    uint32_t *pos, *ord, *len, *run;
    u64 *kp;
};
// kernels/fastq_sort.hip
hipError_t launch_sort_key0(const uint8_t *d_text, const void *d_desc, int by_name, int bytes_only, uint32_t n, uint64_t *d_key,
                            uint32_t *d_val, hipStream_t st);
hipError_t launch_sort_bits(const uint64_t *d_key, uint32_t n, uint64_t *d_bits, int n_cu, hipStream_t st);
hipError_t launch_sort_place0(const void *d_desc, int by_name, const uint32_t *d_val, uint32_t n, uint32_t *d_order, const SortTied &t,
                              hipStream_t st);
hipError_t launch_sort_heads(const uint64_t *d_word, const uint32_t *d_run, uint32_t m, uint32_t *d_head, hipStream_t st);
hipError_t launch_sort_settle(const uint8_t *d_text, const SortTied &t, const uint32_t *d_head, const uint32_t *d_gid, uint32_t c,
                              uint32_t m, int bytes_only, uint32_t *d_stay, uint32_t *d_keep, hipStream_t st);
hipError_t launch_sort_compact(const uint32_t *d_keep, const uint32_t *d_at, const uint32_t *d_head, const uint32_t *d_gid,
                               const SortTied &a, uint32_t m, const SortTied &b, hipStream_t st);
hipError_t launch_sort_word(const uint8_t *d_text, const SortTied &t, uint32_t c, uint32_t m, uint64_t *d_key, uint32_t *d_val,
                            hipStream_t st);
hipError_t launch_sort_runkey(const uint32_t *d_run, const uint32_t *d_val1, uint32_t m, uint64_t *d_key, uint32_t *d_val, hipStream_t st);
hipError_t launch_sort_place(const uint32_t *d_val2, const uint32_t *d_val1, const uint64_t *d_word1, const SortTied &a, uint32_t m,
                             const SortTied &b, uint64_t *d_word, uint32_t *d_order, hipStream_t st);
hipError_t launch_sort_sizes(const void *d_desc, const uint32_t *d_order, uint32_t n, uint32_t *d_size, hipStream_t st);
hipError_t launch_sort_write(const uint8_t *d_text, const void *d_desc, const uint32_t *d_order, const uint64_t *d_off, uint32_t n,
                             uint8_t *d_out, int n_cu, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
constexpr uint32_t kFirstBytes = 6, kWordBytes = 8, kMaxRounds = 128;   // 6 + 8 * 127 = 1022, the longest line gzgets leaves whole
constexpr uint32_t kMaxRoundsKseq = 8194;                               // 6 + 8 * 8192 > 65,535, the longest sequence kseq framing keeps
enum { kSiBits = kInfoOwn };   // the family's words of the info block: two uint64
}  // namespace

struct hpn_sort_work {   // what a new session must not inherit
    Scratch size, off, out;
    uint64_t out_total = 0;
};

struct hpn_sort_state : FamilyState, hpn_sort_work {
    static constexpr int kSlot = kStSort;
    StoreSession s;
    Sorter sorter;
};

namespace {

void drop_session(hpn_sort_state *u)
{
    session_drop(u->s);
    static_cast<hpn_sort_work &>(*u) = hpn_sort_work();
    u->sorter.drop();
}

// Stable sort of (key, val) by the digits in which two of the n keys differ, interior constant digits left out as well.
int sort_differing(hpn_ctx *c, Sorter *u, uint32_t n)
{
    int rc;
    uint64_t *bits = (uint64_t *)(u->info.d + kSiBits);
    HPN_HIP(c, launch_sort_bits((const uint64_t *)u->key.p, n, bits, c->n_cu, c->stream));
    if ((rc = u->info.fetch(c)) != HPN_OK) return rc;
    uint64_t h[2];
    memcpy(h, u->info.h + kSiBits, sizeof h);
    const uint64_t differ = n ? h[0] ^ h[1] : 0;
    uint32_t digits = 0;
    for (int d = 0; d < 8; ++d)
        if ((differ >> (8 * d)) & 255u) digits |= 1u << d;
    if (!digits || n < 2) return HPN_OK;
    const uint64_t hw = uniq_sort_hist_words(n);
    if ((rc = need(c, u->key_tmp, (size_t)n * 8)) != HPN_OK || (rc = need(c, u->val_tmp, (size_t)n * 4)) != HPN_OK ||
        (rc = need(c, u->hist, hw * 4)) != HPN_OK || (rc = need(c, u->offs, hw * 4)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(hw > n ? hw : n) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, uniq_sort_pairs_digits((uint64_t *)u->key.p, (uint32_t *)u->val.p, n, digits, (uint64_t *)u->key_tmp.p, (uint32_t *)u->val_tmp.p,
                                      (uint32_t *)u->hist.p, (uint32_t *)u->offs.p, (u64 *)u->status.p, u->info.ticket(), u->info.err(),
                                      c->stream));
    return HPN_OK;
}

SortTied tied(Sorter *u, int k)
{
    return SortTied{(uint32_t *)u->t_pos[k].p, (uint32_t *)u->t_ord[k].p, (uint32_t *)u->t_len[k].p, (uint32_t *)u->t_run[k].p, (u64 *)u->t_kp[k].p};
}

// The runs of the m tied records of side `cur` whose words (the ones just sorted by) are in `word`: settles what is decided
// behind `c` key bytes and compacts the rest into the other side.  *left: how many stay.
int settle(hpn_ctx *c, Sorter *u, const uint8_t *text, int cur, const uint64_t *word, uint32_t consumed, uint32_t m, uint32_t *left)
{
    int rc;
    if ((rc = need(c, u->status, uniq_scan_tiles(m) * 8)) != HPN_OK) return rc;
    uint32_t *head = (uint32_t *)u->head.p, *gid = (uint32_t *)u->gid.p, *stay = (uint32_t *)u->stay.p, *keep = (uint32_t *)u->keep.p;
    uint32_t *at = (uint32_t *)u->at.p, *ticket = u->info.ticket(), *err = u->info.err();
    const SortTied a = tied(u, cur), b = tied(u, cur ^ 1);
    HPN_HIP(c, launch_sort_heads(word, a.run, m, head, c->stream));
    HPN_HIP(c, uniq_scan32(head, gid, m, (u64 *)u->status.p, ticket, err, c->stream));
    HPN_HIP(c, launch_sort_settle(text, a, head, gid, consumed, m, u->bytes_only, stay, keep, c->stream));
    HPN_HIP(c, uniq_scan32(keep, at, m, (u64 *)u->status.p, ticket, err, c->stream));
    uint32_t n_left = 0;
    HPN_HIP(c, hipMemcpyAsync(&n_left, at + m, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = u->info.fetch(c)) != HPN_OK) return rc;
    if (n_left) HPN_HIP(c, launch_sort_compact(keep, at, head, gid, a, m, b, c->stream));
    *left = n_left;
    return HPN_OK;
}

}  // namespace

int hpn::order_records(hpn_ctx *c, Sorter *u, const uint8_t *text, const void *desc, uint32_t N, hpn_sort_result *res)
{
    int rc;
    const uint32_t max_rounds = u->bytes_only ? kMaxRoundsKseq : kMaxRounds;
    if ((rc = u->info.alloc(c)) != HPN_OK || (rc = u->info.zero(c)) != HPN_OK) return rc;
    if ((rc = need(c, u->order, (size_t)N * 4)) != HPN_OK) return rc;
    if (!N) return HPN_OK;
    Scratch *per4[] = {&u->val, &u->val1, &u->head, &u->stay, &u->keep, &u->t_pos[0], &u->t_pos[1], &u->t_ord[0], &u->t_ord[1],
                       &u->t_len[0], &u->t_len[1], &u->t_run[0], &u->t_run[1]};
    Scratch *per8[] = {&u->key, &u->word1, &u->word, &u->t_kp[0], &u->t_kp[1]};
    for (Scratch *s : per4)
        if ((rc = need(c, *s, (size_t)N * 4)) != HPN_OK) return rc;
    for (Scratch *s : per8)
        if ((rc = need(c, *s, (size_t)N * 8)) != HPN_OK) return rc;
    if ((rc = need(c, u->gid, ((size_t)N + 1) * 4)) != HPN_OK || (rc = need(c, u->at, ((size_t)N + 1) * 4)) != HPN_OK) return rc;
    uint64_t *key = (uint64_t *)u->key.p, *word1 = (uint64_t *)u->word1.p, *word = (uint64_t *)u->word.p;
    uint32_t *val = (uint32_t *)u->val.p, *val1 = (uint32_t *)u->val1.p, *order = (uint32_t *)u->order.p;
    // round 0
    int cur = 0;
    uint32_t m = 0, consumed = kFirstBytes;
    HPN_HIP(c, launch_sort_key0(text, desc, u->by_name, u->bytes_only, N, key, val, c->stream));
    if ((rc = sort_differing(c, u, N)) != HPN_OK) return rc;
    HPN_HIP(c, launch_sort_place0(desc, u->by_name, val, N, order, tied(u, cur), c->stream));
    if ((rc = settle(c, u, text, cur, key, consumed, N, &m)) != HPN_OK) return rc;
    res->rounds = 1;
    while (m) {
        if (res->rounds >= max_rounds) return fail(c, HPN_E_HIP, "the refinement did not end within %u rounds", max_rounds);
        cur ^= 1;   // (settle compacted into the other side)
        res->rounds += 1, res->refined += m;
        const SortTied a = tied(u, cur), b = tied(u, cur ^ 1);
        HPN_HIP(c, launch_sort_word(text, a, consumed, m, key, val, c->stream));
        if ((rc = sort_differing(c, u, m)) != HPN_OK) return rc;
        HPN_HIP(c, hipMemcpyAsync(word1, key, (size_t)m * 8, hipMemcpyDeviceToDevice, c->stream));
        HPN_HIP(c, hipMemcpyAsync(val1, val, (size_t)m * 4, hipMemcpyDeviceToDevice, c->stream));
        HPN_HIP(c, launch_sort_runkey(a.run, val1, m, key, val, c->stream));
        if ((rc = sort_differing(c, u, m)) != HPN_OK) return rc;
        HPN_HIP(c, launch_sort_place(val, val1, word1, a, m, b, word, order, c->stream));
        cur ^= 1;
        consumed += kWordBytes;
        if ((rc = settle(c, u, text, cur, word, consumed, m, &m)) != HPN_OK) return rc;
    }
    return HPN_OK;
}

extern "C" {

int hpn_fastq_sort_begin(hpn_ctx *c, int by_name, uint64_t max_bytes)
{
    if (!c) return HPN_E_ARG;
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_sort_state *u = state_make<hpn_sort_state>(c);
    drop_session(u);
    u->sorter.by_name = by_name ? 1 : 0;
    return session_begin(c, u->s, 1, max_bytes);
}

int hpn_fastq_sort_add(hpn_ctx *c, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_sort_state *u = state<hpn_sort_state>(c);
    return session_add(c, u ? &u->s : nullptr, "hpn_fastq_sort", 0, kSortDescBytes, frame_by<launch_sort_frame>, nullptr, 4u, text, nbytes, last, false, info);
}

int hpn_fastq_sort_finish(hpn_ctx *c, hpn_sort_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_sort_state *u = state<hpn_sort_state>(c);
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_fastq_sort", kSortDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    const uint32_t N = (uint32_t)u->s.m[0].n;
    res->n_records = N;
    uint64_t framed = 0;   // where the last record ends (a last line without '\n': behind the byte it lost)
    if (N) {
        SortDesc d;
        HPN_HIP(c, hipMemcpy(&d, (const SortDesc *)u->s.m[0].desc.p + (N - 1), sizeof d, hipMemcpyDeviceToHost));
        framed = d.off + d.qrel + d.qlen + 1u;
    }
    res->lone_line = framed < u->s.m[0].len ? 1u : 0u;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTally], c->stream));
    if ((rc = order_records(c, &u->sorter, u->s.text(0), u->s.m[0].desc.p, N, res)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTally], c->stream));
    c->ev_valid[kFamTally] = true;
    // the output text
    if ((rc = need(c, u->size, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->off, ((size_t)N + 1) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, launch_sort_sizes(u->s.m[0].desc.p, (const uint32_t *)u->sorter.order.p, N, (uint32_t *)u->size.p, c->stream));
    uint64_t total = 0;
    if ((rc = scan_sizes(c, u->s.info, u->sorter.status, u->size, u->off, N, &total)) != HPN_OK) return rc;
    if ((rc = need(c, u->out, total)) != HPN_OK) return rc;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    HPN_HIP(c, launch_sort_write(u->s.text(0), u->s.m[0].desc.p, (const uint32_t *)u->sorter.order.p, (const uint64_t *)u->off.p, N,
                                 (uint8_t *)u->out.p, c->n_cu, c->stream));
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    HPN_HIP(c, hipStreamSynchronize(c->stream));
    u->out_total = res->out_bytes = total;
    u->s.finished = true;
    return HPN_OK;
}

int hpn_fastq_sort_write(hpn_ctx *c, uint64_t offset, void *out, uint64_t cap, uint64_t *written)
{
    if (!c || !written) return HPN_E_ARG;
    hpn_sort_state *u = state<hpn_sort_state>(c);
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_fastq_sort", written);
    return rc != HPN_OK ? rc : session_write_slice(c, u->out, u->out_total, offset, out, cap, written);
}

}  // extern "C"
