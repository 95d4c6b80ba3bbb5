// hpn_rqcfile.hip -- C ABI of Rfastqc.R's one call, qsort_hash_count(fq1, fq2) of Rgzfastq_uniq.c, from FASTQ text:
// hpn_rfastqc_begin / _add / _finish / _read.  Kernels: kernels/rqc_dedup.hip, the framing of kernels/fastq_sort.hip (k_sort_frame,
// as it is), the scans and the stable radix sort of kernels/fastq_uniq.hip, k_tally_hist and k_read_gc.  The store and its session:
// hpn_store.hpp.
//
// The session is hpn_fastq_pair_*'s front half -- a store per mate, one SortDesc per record -- with another back half.  The domain
// pass (lengths, then bytes) comes first and names the first record the plugin has no answer for.  The lines are gathered into
// the structure-of-arrays buffers the tally kernels take; the matrices are transposed into the plugin's layouts on the device.
// The duplicate counts: hash of the key (kernels/rqc_key.hpp), stable sort, flags over the key's bytes, the host's ordering of
// clashing runs as hpn_uniq_group.hpp does it, a scan, the differences of the group starts, one more sort.  No table is walked
// and no representative is kept: the plugin returns the multiset of counts and nothing else of its table.
#include <algorithm>
#include <string>
#include <vector>

#include "hpn_store.hpp"
#include "kernels/rqc_key.hpp"

namespace hpn {
// kernels/rqc_dedup.hip
hipError_t launch_rqc_sizes(const void *d_desc, uint32_t n, uint32_t mate, uint32_t *d_ssz, uint32_t *d_qsz, uint32_t *d_length, uint32_t *d_info,
                            hipStream_t st);
hipError_t launch_rqc_gather(const uint8_t *d_text, const void *d_desc, uint32_t n, uint32_t mate, const uint64_t *d_soff, const uint64_t *d_qoff,
                             uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_info, int n_cu, hipStream_t st);
hipError_t launch_rqc_key(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, uint32_t n, uint64_t hash_mask,
                          uint64_t *d_hash, uint32_t *d_order, uint8_t *d_klen, int n_cu, hipStream_t st);
hipError_t launch_rqc_flags(const uint8_t *t0, const void *d0, const uint8_t *t1, const void *d1, int paired, const uint64_t *d_hash,
                            const uint32_t *d_order, const uint8_t *d_klen, uint32_t n, uint32_t *d_flag, uint32_t *d_info, int n_cu, hipStream_t st);
hipError_t launch_rqc_counts(const uint32_t *d_flag, const uint32_t *d_gid, uint32_t n, uint32_t n_groups, uint32_t *d_start, uint64_t *d_key,
                             uint32_t *d_val, hipStream_t st);
hipError_t launch_rqc_matrices(const uint64_t *d_acc, int32_t *d_quality, int32_t *d_nucleotide, hipStream_t st);
// kernels/fastq_gc.hip
hipError_t launch_read_gc(const uint8_t *d_seq, const uint64_t *d_off, uint64_t n, double *d_gc, int n_cu, hipStream_t st);
}  // namespace hpn

using namespace hpn;

namespace {
enum { kRqBad = kInfoOwn, kRqRagged, kRqClash };   // the family's words of the info block: what the kernels number 0, 1, 2
enum { kDup = HPN_RFASTQC_DUP, kGc = HPN_RFASTQC_GC, kQuality = HPN_RFASTQC_QUALITY, kNucleotide = HPN_RFASTQC_NUCLEOTIDE, kLength = HPN_RFASTQC_LENGTH, kArrays };
constexpr size_t kLinePad = 16;   // in front of the gathered lines: k_tally_hist reads aligned 16-byte vectors around them
constexpr size_t kAccBytes = (size_t)HPN_TALLY_WORDS * sizeof(uint64_t), kAccBad = HPN_TALLY_W_BAD;   // (plain names: HPN_HIP quotes its call in the message)
constexpr size_t kQualityElems = (size_t)HPN_QUAL_ROWS * kRqcMaxLen, kNucleotideElems = (size_t)HPN_NUC_CODES * kRqcMaxLen;
}  // namespace

struct hpn_rfastqc_work {   // what a new session must not inherit
    Scratch hash, order, klen, flag, gid, start, key, key_tmp, val_tmp, hist, offs, status, ssz[2], qsz[2], soff[2], qoff[2], seq, qual, acc;
    Scratch out[2][kArrays];          // by mate and HPN_RFASTQC_*; the duplicate counts are out[0][kDup]
    uint64_t elems[2][kArrays] = {};
};

struct hpn_rfastqc_state : FamilyState, hpn_rfastqc_work {
    static constexpr int kSlot = kStRfastqc;
    StoreSession s;
    int paired = 0;
    uint32_t hash_bits = 0;
};

namespace {

void drop_session(hpn_rfastqc_state *u)
{
    session_drop(u->s);
    static_cast<hpn_rfastqc_work &>(*u) = hpn_rfastqc_work();
}

int rq_sort(hpn_ctx *c, hpn_rfastqc_state *u, uint64_t *keys, uint32_t *vals, uint32_t n, int end_bit)
{
    int rc;
    const uint64_t hw = uniq_sort_hist_words(n);
    if ((rc = need(c, u->key_tmp, (size_t)n * 8)) != HPN_OK || (rc = need(c, u->val_tmp, (size_t)n * 4)) != HPN_OK ||
        (rc = need(c, u->hist, hw * 4)) != HPN_OK || (rc = need(c, u->offs, hw * 4)) != HPN_OK ||
        (rc = need(c, u->status, uniq_scan_tiles(hw > n ? hw : n) * 8)) != HPN_OK)
        return rc;
    HPN_HIP(c, uniq_sort_pairs(keys, vals, n, 0, end_bit, (uint64_t *)u->key_tmp.p, (uint32_t *)u->val_tmp.p, (uint32_t *)u->hist.p,
                               (uint32_t *)u->offs.p, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
    return HPN_OK;
}

// uniq_order_clashing_runs (hpn_uniq_group.hpp) over this family's descriptors and key rule: runs of equal hashes that hold
// different keys are ordered by the keys' bytes on the host, stably, so equal keys lie side by side.
int order_clashing_runs(hpn_ctx *c, hpn_rfastqc_state *u, uint32_t N)
{
    std::vector<uint8_t> text[2];
    std::vector<SortDesc> desc[2];
    for (int k = 0; k <= u->paired; ++k) {
        text[k].resize(u->s.m[k].len + 1);
        desc[k].resize(N);
        if (u->s.m[k].len) HPN_HIP(c, hipMemcpy(text[k].data(), u->s.text(k), u->s.m[k].len, hipMemcpyDeviceToHost));
        HPN_HIP(c, hipMemcpy(desc[k].data(), u->s.m[k].desc.p, (size_t)N * kSortDescBytes, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> hash(N);
    std::vector<uint32_t> order(N);
    HPN_HIP(c, hipMemcpy(hash.data(), u->hash.p, (size_t)N * 8, hipMemcpyDeviceToHost));
    HPN_HIP(c, hipMemcpy(order.data(), u->order.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    auto key = [&](uint32_t r) {
        const SortDesc &a = desc[0][r];
        uint32_t n0, n1;
        rqc_key_spans(a.slen, u->paired ? desc[1][r].slen : 0u, u->paired, n0, n1);
        std::string s((const char *)text[0].data() + a.off + a.nlen + 1, n0);
        if (n1) s.append((const char *)text[1].data() + desc[1][r].off + desc[1][r].nlen + 1, n1);
        return s;
    };
    for (uint32_t a = 0; a < N;) {
        uint32_t b = a + 1;
        while (b < N && hash[b] == hash[a]) ++b;
        if (b - a > 1) {
            std::vector<std::pair<std::string, uint32_t>> run;
            run.reserve(b - a);
            for (uint32_t i = a; i < b; ++i) run.emplace_back(key(order[i]), order[i]);
            std::stable_sort(run.begin(), run.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
            for (uint32_t i = a; i < b; ++i) order[i] = run[i - a].second;
        }
        a = b;
    }
    HPN_HIP(c, hipMemcpy(u->order.p, order.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    return HPN_OK;
}

// the refusal: names the record, closes the session with nothing to read
int refuse(hpn_ctx *c, hpn_rfastqc_state *u, hpn_rfastqc_result *res, uint32_t bad_key, uint32_t reason)
{
    static const char *const why[] = {"", "has a sequence length outside 1..300: the plugin writes outside its Length vector and matrices",
                                      "has a quality line longer than 300: the plugin writes outside its Quality matrix",
                                      "has a sequence or quality byte >= 128: the plugin indexes with a negative char",
                                      "is missing: mate 2 has fewer records than mate 1 and the plugin dereferences NULL"};
    res->bad_record = (int64_t)(bad_key >> 1), res->bad_mate = bad_key & 1u, res->reason = reason;
    drop_session(u);
    return fail(c, HPN_E_DOMAIN, "record %u (0-based) of mate %u %s", bad_key >> 1, (bad_key & 1u) + 1u, why[reason]);
}

}  // namespace

extern "C" {

int hpn_rfastqc_begin(hpn_ctx *c, int paired, uint64_t max_bytes, uint32_t hash_bits)
{
    if (!c) return HPN_E_ARG;
    if (hash_bits > 63) return fail(c, HPN_E_ARG, "hash_bits %u (0 = all 64, or 1 .. 63)", hash_bits);
    HPN_HIP(c, hipSetDevice(c->device));
    hpn_rfastqc_state *u = state_make<hpn_rfastqc_state>(c);
    drop_session(u);
    u->paired = paired ? 1 : 0, u->hash_bits = hash_bits;
    return session_begin(c, u->s, paired ? 2 : 1, max_bytes);
}

int hpn_rfastqc_add(hpn_ctx *c, int mate, const void *text, uint64_t nbytes, int last, hpn_sort_info *info)
{
    if (!c || !info) return HPN_E_ARG;
    hpn_rfastqc_state *u = state<hpn_rfastqc_state>(c);
    return session_add(c, u ? &u->s : nullptr, "hpn_rfastqc", mate, kSortDescBytes, frame_by<launch_sort_frame>, nullptr, 4u, text, nbytes, last, false, info);
}

int hpn_rfastqc_finish(hpn_ctx *c, hpn_rfastqc_result *res)
{
    if (!c || !res) return HPN_E_ARG;
    hpn_rfastqc_state *u = state<hpn_rfastqc_state>(c);
    int rc;
    if ((rc = session_finish_begin(c, u ? &u->s : nullptr, "hpn_rfastqc", kSortDescBytes)) != HPN_OK) return rc;
    memset(res, 0, sizeof *res);
    res->bad_record = -1;
    const int mates = u->paired + 1;
    const uint32_t N = (uint32_t)u->s.m[0].n, n2 = u->paired ? (uint32_t)u->s.m[1].n : 0u;
    const uint32_t n_mate[2] = {N, n2 < N ? n2 : N};   // mate 2's records behind mate 1's last are never read
    const uint32_t short_key = u->paired && n2 < N ? 2u * n2 + 1u : 0xffffffffu;
    res->n_records = N;
    for (int k = 0; k < mates; ++k) {
        if ((rc = need(c, u->out[k][kQuality], kQualityElems * 4)) != HPN_OK || (rc = need(c, u->out[k][kNucleotide], kNucleotideElems * 4)) != HPN_OK ||
            (rc = need(c, u->out[k][kLength], kRqcMaxLen * 4)) != HPN_OK || (rc = need(c, u->out[k][kGc], (size_t)N * 8)) != HPN_OK)
            return rc;
        HPN_HIP(c, hipMemsetAsync(u->out[k][kQuality].p, 0, kQualityElems * 4, c->stream));
        HPN_HIP(c, hipMemsetAsync(u->out[k][kNucleotide].p, 0, kNucleotideElems * 4, c->stream));
        HPN_HIP(c, hipMemsetAsync(u->out[k][kLength].p, 0, kRqcMaxLen * 4, c->stream));
    }
    if ((rc = need(c, u->out[0][kDup], 4)) != HPN_OK) return rc;
    auto finished = [&](uint64_t n_unique) {
        for (int k = 0; k < mates; ++k)
            u->elems[k][kGc] = N, u->elems[k][kQuality] = kQualityElems, u->elems[k][kNucleotide] = kNucleotideElems, u->elems[k][kLength] = kRqcMaxLen;
        u->elems[0][kDup] = res->n_unique = n_unique;
        u->s.finished = true;
    };
    if (!N) {   // no record: empty vectors, matrices of zeros
        HPN_HIP(c, hipStreamSynchronize(c->stream));
        finished(0);
        return HPN_OK;
    }

    // ---- the domain, lengths first: sizes, Length[], the offsets of the gathered lines
    uint32_t *info = u->s.info.d + kRqBad;
    HPN_HIP(c, hipMemsetAsync(info, 0xff, sizeof(uint32_t), c->stream));
    uint64_t stotal[2] = {0, 0}, qtotal[2] = {0, 0};
    for (int k = 0; k < mates; ++k) {
        const uint32_t n = n_mate[k];
        if ((rc = need(c, u->ssz[k], (size_t)n * 4)) != HPN_OK || (rc = need(c, u->qsz[k], (size_t)n * 4)) != HPN_OK ||
            (rc = need(c, u->soff[k], ((size_t)n + 1) * 8)) != HPN_OK || (rc = need(c, u->qoff[k], ((size_t)n + 1) * 8)) != HPN_OK)
            return rc;
        HPN_HIP(c, launch_rqc_sizes(u->s.m[k].desc.p, n, (uint32_t)k, (uint32_t *)u->ssz[k].p, (uint32_t *)u->qsz[k].p, (uint32_t *)u->out[k][kLength].p,
                                    info, c->stream));
        if (!n) continue;   // (mate 2 without a record: refused below)
        if ((rc = scan_sizes(c, u->s.info, u->status, u->ssz[k], u->soff[k], n, &stotal[k])) != HPN_OK ||
            (rc = scan_sizes(c, u->s.info, u->status, u->qsz[k], u->qoff[k], n, &qtotal[k])) != HPN_OK)
            return rc;
    }
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    if (u->s.info.h[kRqBad] < short_key) {
        const uint32_t bad = u->s.info.h[kRqBad];
        SortDesc d;
        HPN_HIP(c, hipMemcpy(&d, (const uint8_t *)u->s.m[bad & 1u].desc.p + (size_t)(bad >> 1) * kSortDescBytes, kSortDescBytes, hipMemcpyDeviceToHost));
        return refuse(c, u, res, bad, d.slen < 1u || d.slen > kRqcMaxLen ? HPN_RFASTQC_BAD_LENGTH : HPN_RFASTQC_BAD_QUALITY);
    }
    const bool ragged = u->s.info.h[kRqRagged] != 0;

    // ---- the lines gathered, the bytes' domain on the way; matrices and GC per mate
    uint64_t most_s = stotal[0] > stotal[1] ? stotal[0] : stotal[1], most_q = qtotal[0] > qtotal[1] ? qtotal[0] : qtotal[1];
    if ((rc = need(c, u->seq, kLinePad + most_s)) != HPN_OK || (rc = need(c, u->qual, kLinePad + most_q)) != HPN_OK || (rc = need(c, u->acc, kAccBytes)) != HPN_OK)
        return rc;
    uint8_t *seq = (uint8_t *)u->seq.p + kLinePad, *qual = (uint8_t *)u->qual.p + kLinePad;
    u64 *acc = (u64 *)u->acc.p;
    uint64_t tally_bad[2] = {0, 0};
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTrim], c->stream));
    for (int k = 0; k < mates; ++k) {
        const uint32_t n = n_mate[k];
        if (!n) continue;
        const uint64_t *soff = (const uint64_t *)u->soff[k].p, *qoff = (const uint64_t *)u->qoff[k].p;
        HPN_HIP(c, launch_rqc_gather(u->s.text(k), u->s.m[k].desc.p, n, (uint32_t)k, soff, qoff, seq, qual, info, c->n_cu, c->stream));
        HPN_HIP(c, hipMemsetAsync(acc, 0, kAccBytes, c->stream));
        if (!ragged) {
            HPN_HIP(c, launch_tally_hist(qual, seq, soff, n, true, true, acc, c->n_cu, c->stream));
        } else {   // each kind of line against its own offsets
            HPN_HIP(c, launch_tally_hist(qual, nullptr, qoff, n, true, false, acc, c->n_cu, c->stream));
            HPN_HIP(c, launch_tally_hist(nullptr, seq, soff, n, false, true, acc, c->n_cu, c->stream));
        }
        HPN_HIP(c, launch_rqc_matrices((const uint64_t *)acc, (int32_t *)u->out[k][kQuality].p, (int32_t *)u->out[k][kNucleotide].p, c->stream));
        HPN_HIP(c, hipMemcpyAsync(&tally_bad[k], acc + kAccBad, 8, hipMemcpyDeviceToHost, c->stream));
        HPN_HIP(c, launch_read_gc(seq, soff, n, (double *)u->out[k][kGc].p, c->n_cu, c->stream));
    }
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTrim], c->stream));
    c->ev_valid[kFamTrim] = true;
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    const uint32_t bad = u->s.info.h[kRqBad] < short_key ? u->s.info.h[kRqBad] : short_key;
    if (bad != 0xffffffffu) return refuse(c, u, res, bad, bad == short_key ? HPN_RFASTQC_MATE_SHORT : HPN_RFASTQC_BAD_BYTE);
    if (tally_bad[0] || tally_bad[1]) {
        drop_session(u);
        return fail(c, HPN_E_DOMAIN, "the tally kernel refused lines that passed the domain pass");
    }

    // ---- the duplicate counts
    if ((rc = need(c, u->hash, (size_t)N * 8)) != HPN_OK || (rc = need(c, u->order, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->klen, N)) != HPN_OK ||
        (rc = need(c, u->flag, (size_t)N * 4)) != HPN_OK || (rc = need(c, u->gid, ((size_t)N + 1) * 4)) != HPN_OK)
        return rc;
    const uint8_t *t0 = u->s.text(0), *t1 = u->paired ? u->s.text(1) : nullptr;
    const void *d0 = u->s.m[0].desc.p, *d1 = u->paired ? u->s.m[1].desc.p : nullptr;
    uint64_t *hash = (uint64_t *)u->hash.p;
    uint32_t *order = (uint32_t *)u->order.p, *flag = (uint32_t *)u->flag.p, *gid = (uint32_t *)u->gid.p;
    uint8_t *klen = (uint8_t *)u->klen.p;
    const uint64_t mask = u->hash_bits ? (1ull << u->hash_bits) - 1 : ~0ull;
    HPN_HIP(c, hipEventRecord(c->ev_beg[kFamTally], c->stream));
    HPN_HIP(c, launch_rqc_key(t0, d0, t1, d1, u->paired, N, mask, hash, order, klen, c->n_cu, c->stream));
    if ((rc = rq_sort(c, u, hash, order, N, u->hash_bits ? (int)u->hash_bits : 64)) != HPN_OK) return rc;
    HPN_HIP(c, launch_rqc_flags(t0, d0, t1, d1, u->paired, hash, order, klen, N, flag, info, c->n_cu, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    res->hash_clashes = u->s.info.h[kRqClash];
    if (res->hash_clashes) {
        if ((rc = order_clashing_runs(c, u, N)) != HPN_OK) return rc;
        HPN_HIP(c, launch_rqc_flags(t0, d0, t1, d1, u->paired, hash, order, klen, N, flag, info, c->n_cu, c->stream));
    }
    if ((rc = need(c, u->status, uniq_scan_tiles(N) * 8)) != HPN_OK) return rc;
    HPN_HIP(c, uniq_scan32(flag, gid, N, (u64 *)u->status.p, u->s.info.ticket(), u->s.info.err(), c->stream));
    uint32_t U = 0;
    HPN_HIP(c, hipMemcpyAsync(&U, gid + N, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    if ((rc = need(c, u->start, ((size_t)U + 1) * 4)) != HPN_OK || (rc = need(c, u->key, (size_t)U * 8)) != HPN_OK ||
        (rc = need(c, u->out[0][kDup], (size_t)U * 4)) != HPN_OK)
        return rc;
    uint32_t *dup = (uint32_t *)u->out[0][kDup].p;
    HPN_HIP(c, launch_rqc_counts(flag, gid, N, U, (uint32_t *)u->start.p, (uint64_t *)u->key.p, dup, c->stream));
    if ((rc = rq_sort(c, u, (uint64_t *)u->key.p, dup, U, 32 - __builtin_clz(N))) != HPN_OK) return rc;   // keys are N - count < N
    HPN_HIP(c, hipEventRecord(c->ev_end[kFamTally], c->stream));
    c->ev_valid[kFamTally] = true;
    if ((rc = u->s.info.fetch(c)) != HPN_OK) return rc;
    finished(U);
    return HPN_OK;
}

int hpn_rfastqc_read(hpn_ctx *c, int which, int mate, uint64_t first_elem, void *out, uint64_t cap_elems, uint64_t *got)
{
    if (!c || !got) return HPN_E_ARG;
    hpn_rfastqc_state *u = state<hpn_rfastqc_state>(c);
    const int rc = session_write_begin(c, u ? &u->s : nullptr, "hpn_rfastqc", got);
    if (rc != HPN_OK) return rc;
    if (which < kDup || which > kLength) return fail(c, HPN_E_ARG, "array %d (0 dup, 1 gc, 2 quality, 3 nucleotide, 4 length)", which);
    if (which == kDup) mate = 0;
    if (mate < 0 || mate > u->paired) return fail(c, HPN_E_ARG, "mate %d of a %s session", mate, u->paired ? "paired" : "single-end");
    const uint64_t total = u->elems[mate][which], es = which == kGc ? 8 : 4;
    if (first_elem > total) return fail(c, HPN_E_ARG, "element %llu beyond the array's %llu", (unsigned long long)first_elem, (unsigned long long)total);
    if (cap_elems > total - first_elem) cap_elems = total - first_elem;
    uint64_t bytes = 0;
    const int wrc = session_write_slice(c, u->out[mate][which], total * es, first_elem * es, out, cap_elems * es, &bytes);
    *got = bytes / es;
    return wrc;
}

}  // extern "C"
