// bam_view.hip -- samtools view (sam_view.c, bam.c of samtools-0.1.19) on the device: the filters of process_aln as a keep bit per
// record, and bam_format1_core's SAM line as a length first and bytes later.  (docs/kernels/bam_view.md)
//
//   k_view_classify  16 lanes a record, in place through rec_off[] (hpn_bam_raw_index_dev): size 4 + block_size, where the record
//                    lies in the session's store; the keep bit -- flag, mapq and the -m CIGAR sum by the team's first lane, the
//                    name's X31 hash as a polynomial in 31 over the 16 lanes --; for text sessions the line's exact length, the
//                    aux fields walked by the first lane; and the domain checks
//   k_view_compact   order[] of the kept records from the scan of the keep bits
//   k_view_klen      the kept lines' lengths, 64 bits wide, for the scan that places them
//   k_view_format    16 lanes an output record: the first lane writes the head fields, the CIGAR and the aux fields, the team the
//                    sequence and the quality line.  Plain byte stores inside [line start, line end).
//   k_view_qscale    16 lanes a gathered record: -Q's min(q * scale, 93) over the quality bytes, in front of the cuts and the CRC-32
// No kernel waits for another workgroup.
#include "bam_view.hpp"
#include "common.hpp"

namespace hpn {

namespace {

__device__ __forceinline__ uint32_t vw_word(const uint8_t *q)      // (records are not aligned: bytes)
{
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
}

__device__ __forceinline__ uint32_t vw_digits(uint32_t v)          // decimal digits of v (1 for 0): kputuw
{
    uint32_t d = 1;
    for (; v >= 10u; v /= 10u) ++d;
    return d;
}

__device__ __forceinline__ uint32_t vw_digits_signed(int32_t v)    // kputw: a '-' in front of a negative number
{
    const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    return vw_digits(mag) + (v < 0 ? 1u : 0u);
}

__device__ __forceinline__ uint32_t vw_pow31(uint32_t e)           // 31^e modulo 2^32
{
    uint32_t r = 1, b = 31;
    for (; e; e >>= 1, b *= b)
        if (e & 1u) r *= b;
    return r;
}

__device__ __forceinline__ u64 vw_wave_min64(u64 v)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const u64 o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

// the value of an integer aux field of type t at s as kputw / kputuw print it: its digits and sign
__device__ __forceinline__ uint32_t vw_int_size(uint8_t t)
{
    return t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : t == 'i' || t == 'I' ? 4u : 0u;
}

__device__ __forceinline__ void vw_int_value(uint8_t t, const uint8_t *s, bool &neg, uint32_t &mag)
{
    int32_t v;
    switch (t) {
    case 'c': v = (int8_t)s[0]; break;
    case 'C': v = s[0]; break;
    case 's': v = (int16_t)((uint32_t)s[0] | (uint32_t)s[1] << 8); break;
    case 'S': v = (int32_t)((uint32_t)s[0] | (uint32_t)s[1] << 8); break;
    case 'I': neg = false, mag = vw_word(s); return;
    default: v = (int32_t)vw_word(s); break;
    }
    neg = v < 0, mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
}

// bam_format1_core's walk over the aux fields [s, end): the bytes of their text, or the reason the walk is not the device's
__device__ uint32_t vw_aux_len(const uint8_t *s, const uint8_t *end, u64 &len)
{
    while (s < end) {
        if (end - s < 3) return kVwrLayout;
        const uint8_t type = s[2];
        s += 3, len += 4;                          // a tab, the key, a colon
        const uint32_t w = vw_int_size(type);
        bool neg;
        uint32_t mag;
        if (w) {
            if ((uint64_t)(end - s) < w) return kVwrLayout;
            vw_int_value(type, s, neg, mag);
            len += 2u + vw_digits(mag) + (neg ? 1u : 0u), s += w;
        } else if (type == 'A') {
            if (end - s < 1) return kVwrLayout;
            if (!*s) return kVwrANul;
            len += 3, ++s;
        } else if (type == 'f' || type == 'd') {
            return kVwrFloat;
        } else if (type == 'Z' || type == 'H') {
            len += 2;
            while (s < end && *s) ++s, ++len;
            if (s >= end) return kVwrLayout;
            ++s;
        } else if (type == 'B') {
            if (end - s < 5) return kVwrLayout;
            const uint8_t sub = s[0];
            const int32_t n = (int32_t)vw_word(s + 1);
            s += 5, len += 3;
            if (sub == 'f') return kVwrFloat;
            const uint32_t sw = vw_int_size(sub);
            if (!sw || n < 0) return kVwrAuxType;
            if ((uint64_t)(end - s) < (uint64_t)n * sw) return kVwrLayout;
            for (int32_t k = 0; k < n; ++k, s += sw) {
                vw_int_value(sub, s, neg, mag);
                len += 1u + vw_digits(mag) + (neg ? 1u : 0u);
            }
        } else {
            return kVwrAuxType;
        }
    }
    return 0;
}

// bam_aux_get(b, "RG") over the aux fields [s, end), with __skip_tag's sizes (the type upper-cased first, so `d` has size 0 like
// every type it does not know; a B array's subtype as it is): *val the C string behind the field's type byte, nullptr where there
// is no RG field; the reason where the walk or the value leaves the record
__device__ __forceinline__ uint32_t vw_rg_width(uint8_t t)
{
    return t == 'C' || t == 'c' || t == 'A' ? 1u : t == 'S' || t == 's' ? 2u : t == 'I' || t == 'i' || t == 'f' || t == 'F' ? 4u : 0u;
}

__device__ uint32_t vw_aux_rg(const uint8_t *s, const uint8_t *end, const uint8_t **val)
{
    *val = nullptr;
    while (s < end) {
        if (end - s < 2) return kVwrLayout;
        const bool rg = s[0] == 'R' && s[1] == 'G';
        s += 2;
        if (rg) {
            const uint8_t *e = s + 1;
            while (e < end && *e) ++e;
            if (e >= end) return kVwrLayout;
            *val = s + 1;
            return 0;
        }
        if (s >= end) return kVwrLayout;
        uint8_t t = *s++;
        if (t >= 'a' && t <= 'z') t = (uint8_t)(t - 32);
        if (t == 'Z' || t == 'H') {
            while (s < end && *s) ++s;
            if (s >= end) return kVwrLayout;
            ++s;
        } else if (t == 'B') {
            if (end - s < 5) return kVwrLayout;
            const int32_t n = (int32_t)vw_word(s + 1);
            if (n < 0) return kVwrLayout;
            const uint64_t step = 5ull + (uint64_t)vw_rg_width(s[0]) * (uint64_t)n;
            if (step >= (uint64_t)(end - s)) return 0;
            s += step;
        } else {
            const uint32_t w = vw_rg_width(t);
            if (w >= (uint64_t)(end - s)) return 0;
            s += w;
        }
    }
    return 0;
}

// the C string v against the IDs [a, b) of the table
__device__ __forceinline__ bool vw_id_in(const uint8_t *v, const VwRules &r, uint32_t a, uint32_t b)
{
    for (uint32_t k = a; k < b; ++k) {
        const uint8_t *id = r.ids + r.id_off[k];
        const uint32_t len = r.id_off[k + 1] - r.id_off[k];
        uint32_t j = 0;
        while (j < len && v[j] && v[j] == id[j]) ++j;
        if (j == len && !v[j]) return true;
    }
    return false;
}

// a writer that never leaves [w, lim): what does not fit is dropped (the length was computed from the same bytes)
struct VwText {
    uint8_t *w, *lim;
    __device__ __forceinline__ void put(uint8_t c)
    {
        if (w < lim) *w = c;
        ++w;
    }
    __device__ __forceinline__ void number(bool neg, uint32_t mag)
    {
        uint8_t buf[10];
        int l = 0;
        do buf[l++] = (uint8_t)('0' + mag % 10u), mag /= 10u;
        while (mag);
        if (neg) put('-');
        while (l) put(buf[--l]);
    }
    __device__ __forceinline__ void number(int32_t v) { number(v < 0, v < 0 ? 0u - (uint32_t)v : (uint32_t)v); }
    __device__ __forceinline__ void bytes(const uint8_t *p, uint32_t n)
    {
        for (uint32_t k = 0; k < n; ++k) put(p[k]);
    }
};

__device__ __forceinline__ uint32_t vw_flag_len(uint32_t flag, uint32_t style)
{
    if (style == kVwDec) return vw_digits(flag);
    if (style == kVwHex) {
        uint32_t d = 1;
        for (uint32_t v = flag; v >= 16u; v >>= 4) ++d;
        return 2u + d;
    }
    return (uint32_t)__popc(flag & 0x7ffu);        // bam_flag2char_table: "pPuUrR12sfd", nothing above bit 10
}

__device__ __forceinline__ void vw_aux_text(VwText &t, const uint8_t *s, const uint8_t *end)
{
    while (s < end) {                              // (classified: every field ends inside the record)
        const uint8_t type = s[2];
        t.put('\t'), t.put(s[0]), t.put(s[1]), t.put(':');
        s += 3;
        const uint32_t w = vw_int_size(type);
        bool neg;
        uint32_t mag;
        if (w) {
            vw_int_value(type, s, neg, mag);
            t.put('i'), t.put(':'), t.number(neg, mag), s += w;
        } else if (type == 'A') {
            t.put('A'), t.put(':'), t.put(*s++);
        } else if (type == 'Z' || type == 'H') {
            t.put(type), t.put(':');
            while (s < end && *s) t.put(*s++);
            ++s;
        } else if (type == 'B') {
            const uint8_t sub = s[0];
            const int32_t n = (int32_t)vw_word(s + 1);
            const uint32_t sw = vw_int_size(sub);
            s += 5;
            t.put('B'), t.put(':'), t.put(sub);
            if (!sw) return;
            for (int32_t k = 0; k < n && s + sw <= end; ++k, s += sw) {
                vw_int_value(sub, s, neg, mag);
                t.put(','), t.number(neg, mag);
            }
        } else {
            return;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kVwThreads) void k_view_classify(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                              uint64_t base, uint64_t store_at, VwRules r, uint32_t *__restrict__ size,
                                                              u64 *__restrict__ soff, uint32_t *__restrict__ keep, uint32_t *__restrict__ llen,
                                                              u64 *__restrict__ info)
{
    const uint64_t i = ((uint64_t)blockIdx.x * kVwThreads + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    const bool text = r.emit == kVwText, live = i < n;
    u64 bad = ~0ull;
    uint32_t hash = 0, bs = 0, l_qname = 0;
    uint64_t o = 0;
    const uint8_t *q = raw;
    bool named = false;                            // the name lies inside the record and is read
    if (live) {
        o = rec_off[i], q = raw + o;
        bs = vw_word(q), l_qname = q[12];
        named = (text || r.subsample) && l_qname != 0 && 32ull + l_qname <= bs;
    }
    // X31 over the name's l_qname - 1 bytes: sum of s[k] * 31^(L - 1 - k), the bytes as signed chars; a NUL among them is seen
    uint32_t nul_inside = 0;
    if (named) {
        const uint32_t L = l_qname - 1u;
        for (uint32_t k = sub; k < L; k += 16u) {
            const uint8_t c = q[36 + k];
            nul_inside |= c == 0 ? 1u : 0u;
            hash += (uint32_t)(int32_t)(int8_t)c * vw_pow31(L - 1u - k);
        }
    }
#pragma unroll
    for (int d = 1; d < 16; d *= 2) hash += __shfl_xor(hash, d, kWave), nul_inside |= __shfl_xor(nul_inside, d, kWave);
    if (live && sub == 0) {
        const uint32_t tid = vw_word(q + 4), pos = vw_word(q + 8), mapq = q[13], fn = vw_word(q + 16), l_qseq = vw_word(q + 20);
        const uint32_t mtid = vw_word(q + 24), mpos = vw_word(q + 28), isize = vw_word(q + 32);
        const uint32_t n_cigar = fn & 0xffffu, flag = fn >> 16;
        const bool walks = text || r.subsample || r.min_qlen > 0 || r.qual_scale > 1 || r.rg_rule;      // the record's inside is looked at
        uint32_t reason = 0, kept = 1;
        u64 len = 0;
        const u64 fixed = 32ull + l_qname + 4ull * n_cigar, seq_bytes = ((u64)l_qseq + 1) / 2 + l_qseq;
        if (walks && (bs < 32u || (int32_t)l_qseq < 0 || fixed + seq_bytes > bs || l_qname == 0)) {
            reason = kVwrLayout;
        } else {
            if (named && (nul_inside || q[36 + l_qname - 1] != 0)) reason = kVwrName;
            const uint8_t *cg = q + 36 + l_qname;
            if (r.min_qlen > 0) {                  // -m: ops whose type has bit 1, and H
                uint32_t qlen = 0;
                for (uint32_t k = 0; k < n_cigar; ++k) {
                    const uint32_t c = vw_word(cg + 4 * (size_t)k), op = c & 15u;
                    if ((0x3C1A7u >> (op << 1) & 1u) || op == 5u) qlen += c >> 4;
                }
                if ((int32_t)qlen < r.min_qlen) kept = 0;
            }
            if (mapq < r.min_mapq || (flag & r.flag_on) != r.flag_on || (flag & r.flag_off)) kept = 0;
            if (r.subsample && ((hash + r.seed) & 0xffffffu) >= r.threshold) kept = 0;
            if (r.rg_rule && kept && !reason) {    // process_aln's last two steps, for a record the filters in front let through
                const uint8_t *v;
                reason = vw_aux_rg(cg + 4 * (size_t)n_cigar + (l_qseq + 1u) / 2u + l_qseq, q + 4 + bs, &v);
                if (!reason) {
                    if (v && (r.rg_rule & kVwRuleId)) kept = vw_id_in(v, r, 0, r.n_r) ? 1u : 0u;
                    else if (v && (r.rg_rule & kVwRuleSet)) kept = vw_id_in(v, r, r.n_r, r.n_r + r.n_R) ? 1u : 0u;
                    else if (r.rg_rule & kVwRuleLib) kept = v && vw_id_in(v, r, r.n_r + r.n_R, r.n_r + r.n_R + r.n_l) ? 1u : 0u;
                }
            }
            if (text && !reason) {
                if (pos == 0x7fffffffu || mpos == 0x7fffffffu) reason = kVwrPos;
                if (((int32_t)tid >= 0 && tid >= r.n_targets) || ((int32_t)mtid >= 0 && mtid != tid && mtid >= r.n_targets)) reason = kVwrTarget;
            }
            if (text && !reason) {
                len = (u64)l_qname - 1 + 1 + vw_flag_len(flag, r.flag_style) + 1;
                len += (int32_t)tid < 0 ? 2u : r.name_off[tid + 1] - r.name_off[tid] + 1u;
                len += vw_digits_signed((int32_t)(pos + 1u)) + 1u + vw_digits(mapq) + 1u;
                if (!n_cigar) len += 1;
                for (uint32_t k = 0; k < n_cigar; ++k) {
                    const uint32_t c = vw_word(cg + 4 * (size_t)k);
                    if ((c & 15u) > 9u) reason = kVwrCigarOp;
                    len += vw_digits(c >> 4) + 1u;
                }
                len += 1;
                len += (int32_t)mtid < 0 || mtid == tid ? 2u : r.name_off[mtid + 1] - r.name_off[mtid] + 1u;
                len += vw_digits_signed((int32_t)(mpos + 1u)) + 1u + vw_digits_signed((int32_t)isize) + 1u;
                const uint8_t *ql = cg + 4 * (size_t)n_cigar + (l_qseq + 1u) / 2u;
                if (!l_qseq) len += 3;
                else len += (u64)l_qseq + 1 + (ql[0] == 0xffu && r.qual_scale <= 1 ? 1u : l_qseq);
                if (!reason) reason = vw_aux_len(ql + l_qseq, q + 4 + bs, len);
                len += 1;                          // the newline
                if (len > 0xffffffffull) reason = kVwrLayout;
            }
        }
        if (reason) bad = (base + i) << kVwReasonBits | reason;
        size[base + i] = bs + 4u;
        soff[base + i] = store_at + (o - rec_off[0]);
        keep[base + i] = kept;
        llen[base + i] = (uint32_t)len;
        if (i == 0) info[kBsFirst] = o;
        if (i == n - 1) info[kBsEnd] = o + 4 + (uint64_t)bs;
    }
    bad = vw_wave_min64(bad);
    if (lane_id() == 0 && bad != ~0ull) atomicMin(&info[kBsBad], bad);
}

__global__ __launch_bounds__(kVwThreads) void k_view_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kidx, uint64_t n,
                                                             uint32_t *__restrict__ order)
{
    const uint64_t i = (uint64_t)blockIdx.x * kVwThreads + threadIdx.x;
    if (i < n && keep[i]) order[kidx[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(kVwThreads) void k_view_klen(const uint32_t *__restrict__ llen, const uint32_t *__restrict__ order, uint64_t n_out,
                                                          u64 *__restrict__ klen)
{
    const uint64_t j = (uint64_t)blockIdx.x * kVwThreads + threadIdx.x;
    if (j < n_out) klen[j] = llen[order[j]];
}

__global__ __launch_bounds__(kVwThreads) void k_view_format(const uint8_t *__restrict__ store, const u64 *__restrict__ soff,
                                                            const uint32_t *__restrict__ size, const uint32_t *__restrict__ order,
                                                            const u64 *__restrict__ toff, uint64_t first, uint64_t cnt, VwRules r,
                                                            uint8_t *__restrict__ text)
{
    const uint64_t k = ((uint64_t)blockIdx.x * kVwThreads + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    const bool live = k < cnt;
    const uint8_t *q = store;
    uint8_t *line = text, *lim = text;
    uint32_t bs = 0, l_qname = 1, n_cigar = 0, l_qseq = 0;
    if (live) {
        const uint32_t i = order[first + k];
        q = store + soff[i];
        bs = size[i] - 4u, l_qname = q[12], n_cigar = vw_word(q + 16) & 0xffffu, l_qseq = vw_word(q + 20);
        line = text + (toff[first + k] - toff[first]), lim = text + (toff[first + k + 1] - toff[first]);
    }
    const uint8_t *cg = q + 36 + l_qname, *sq = cg + 4 * (size_t)n_cigar, *ql = sq + (l_qseq + 1u) / 2u;
    VwText t = {line, lim};
    if (live && sub == 0) {
        const uint32_t tid = vw_word(q + 4), pos = vw_word(q + 8), mapq = q[13], flag = vw_word(q + 16) >> 16;
        const uint32_t mtid = vw_word(q + 24), mpos = vw_word(q + 28), isize = vw_word(q + 32);
        t.bytes(q + 36, l_qname - 1u), t.put('\t');
        if (r.flag_style == kVwDec) {
            t.number(false, flag);
        } else if (r.flag_style == kVwHex) {
            t.put('0'), t.put('x');
            int sh = 12;
            while (sh && !(flag >> sh)) sh -= 4;
            for (; sh >= 0; sh -= 4) t.put((uint8_t)"0123456789abcdef"[flag >> sh & 15u]);
        } else {
            for (uint32_t b = 0; b < 11u; ++b)
                if (flag >> b & 1u) t.put((uint8_t)"pPuUrR12sfd"[b]);
        }
        t.put('\t');
        if ((int32_t)tid < 0) t.put('*');
        else t.bytes(r.names + r.name_off[tid], r.name_off[tid + 1] - r.name_off[tid]);
        t.put('\t'), t.number((int32_t)(pos + 1u)), t.put('\t'), t.number(false, mapq), t.put('\t');
        if (!n_cigar) t.put('*');
        for (uint32_t c = 0; c < n_cigar; ++c) {
            const uint32_t w = vw_word(cg + 4 * (size_t)c);
            t.number(false, w >> 4), t.put((uint8_t)"MIDNSHP=XB??????"[w & 15u]);
        }
        t.put('\t');
        if ((int32_t)mtid < 0) t.put('*');
        else if (mtid == tid) t.put('=');
        else t.bytes(r.names + r.name_off[mtid], r.name_off[mtid + 1] - r.name_off[mtid]);
        t.put('\t'), t.number((int32_t)(mpos + 1u)), t.put('\t'), t.number((int32_t)isize), t.put('\t');
    }
    // where the sequence starts: the first lane knows, the team reads it from there
    const uint64_t at = __shfl((uint64_t)(t.w - line), 0, 16);
    uint8_t *w = line + at;
    const bool absent = l_qseq && ql[0] == 0xffu && r.qual_scale <= 1;
    if (live && l_qseq) {
        for (uint32_t b = sub; b < l_qseq; b += 16u)
            if (w + b < lim) w[b] = (uint8_t)"=ACMGRSVTWYHKDBN"[sq[b >> 1] >> ((~b & 1u) << 2) & 15u];
        uint8_t *v = w + l_qseq + 1;
        if (!absent)
            for (uint32_t b = sub; b < l_qseq; b += 16u) {
                uint32_t c = ql[b];
                if (r.qual_scale > 1) c = (u64)c * (u64)r.qual_scale < 93ull ? c * (uint32_t)r.qual_scale : 93u;
                if (v + b < lim) v[b] = (uint8_t)(c + 33u);
            }
    }
    if (live && sub == 0) {
        if (!l_qseq) {
            t.put('*'), t.put('\t'), t.put('*');
        } else {
            t.w = w + l_qseq, t.put('\t');
            if (absent) t.put('*');
            else t.w += l_qseq;
        }
        vw_aux_text(t, ql + l_qseq, q + 4 + bs);
        t.put('\n');
    }
}

__global__ __launch_bounds__(kVwThreads) void k_view_qscale(const u64 *__restrict__ out_off, uint64_t first, uint64_t cnt, int32_t scale,
                                                            uint8_t *__restrict__ pay)
{
    const uint64_t k = ((uint64_t)blockIdx.x * kVwThreads + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (k >= cnt) return;
    uint8_t *d = pay + (out_off[first + k] - out_off[first]);
    const uint64_t len = out_off[first + k + 1] - out_off[first + k];
    const uint32_t l_qname = d[12], n_cigar = vw_word(d + 16) & 0xffffu, l_qseq = vw_word(d + 20);
    const uint64_t at = 36ull + l_qname + 4ull * n_cigar + ((uint64_t)l_qseq + 1) / 2;
    if ((int32_t)l_qseq < 0 || at + l_qseq > len) return;      // (classified: it lies inside)
    for (uint32_t b = sub; b < l_qseq; b += 16u) {
        const u64 c = (u64)d[at + b] * (u64)scale;     // 64 bits, as the host route: no scale wraps
        d[at + b] = (uint8_t)(c < 93ull ? c : 93ull);
    }
}

static inline unsigned vw_grid(uint64_t n) { return (unsigned)((n + kVwThreads - 1) / kVwThreads); }

hipError_t launch_bamview_classify(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, VwRules r, uint32_t *size,
                                   u64 *soff, uint32_t *keep, uint32_t *llen, u64 *info, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_view_classify, dim3(vw_grid(n * 16)), dim3(kVwThreads), 0, st, raw, rec_off, n, base, store_at, r, size, soff, keep, llen, info);
    return hipGetLastError();
}

hipError_t launch_bamview_compact(const uint32_t *keep, const uint32_t *kidx, uint64_t n, uint32_t *order, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_view_compact, dim3(vw_grid(n)), dim3(kVwThreads), 0, st, keep, kidx, n, order);
    return hipGetLastError();
}

hipError_t launch_bamview_klen(const uint32_t *llen, const uint32_t *order, uint64_t n_out, u64 *klen, hipStream_t st)
{
    if (!n_out) return hipSuccess;
    hipLaunchKernelGGL(k_view_klen, dim3(vw_grid(n_out)), dim3(kVwThreads), 0, st, llen, order, n_out, klen);
    return hipGetLastError();
}

hipError_t launch_bamview_format(const uint8_t *store, const u64 *soff, const uint32_t *size, const uint32_t *order, const u64 *toff, uint64_t first,
                                 uint64_t cnt, VwRules r, uint8_t *text, hipStream_t st)
{
    if (!cnt) return hipSuccess;
    hipLaunchKernelGGL(k_view_format, dim3(vw_grid(cnt * 16)), dim3(kVwThreads), 0, st, store, soff, size, order, toff, first, cnt, r, text);
    return hipGetLastError();
}

hipError_t launch_bamview_qscale(const u64 *out_off, uint64_t first, uint64_t cnt, int32_t scale, uint8_t *pay, hipStream_t st)
{
    if (!cnt) return hipSuccess;
    hipLaunchKernelGGL(k_view_qscale, dim3(vw_grid(cnt * 16)), dim3(kVwThreads), 0, st, out_off, first, cnt, scale, pay);
    return hipGetLastError();
}

}  // namespace hpn
