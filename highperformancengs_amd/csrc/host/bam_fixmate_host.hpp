// bam_fixmate_host.hpp -- samtools-0.1.19's `fixmate` on the host: the options and bam_mating_core's state machine itself over a
// streaming reader -- one pending record, bam_calend with its backward walk for the B op, the 0x4 update against the target's
// length, the pair and singleton fixes, bam_template_cigar's CT field with kputw's digits -- written through bam_write1's cuts.
// The route of HPN_BAM_GPU=0, of stdin and stdout, and the fallback of bin/bam_fixmate outside the device's domain (a CIGAR op
// above 8, a NUL inside a name).  (docs/kernels/bam_fixmate.md states the rules; tests/fixmate_ref.py is the same in Python,
// tests/golden/fixmate/ the recorded runs.)
//
// Where the reference would read memory that is not its own -- a refID the header does not have (target_len[tid]), a CIGAR op
// above 10 in a CT field (BAM_CIGAR_STR ends at its NUL, op 10), a name or CIGAR past its record -- Undefined is thrown: the tool
// says so under [hpn], leaves with status 2 and no output.  Nothing here needs a GPU: tests/fixmate_host_main.cpp builds this
// header alone.
#pragma once
#include "bam_sort_host.hpp"

namespace hpn {
namespace fixmate {

struct Options {
    bool remove_reads = false;
    const char *in = nullptr, *out = nullptr;
};

struct Undefined {
    std::string what;
};

// bam_mating's own argument handling; false: fewer than two arguments remain (the usage text has been printed, status 1)
inline bool parse_args(int argc, char *argv[], Options &o)
{
    int c;
    while ((c = getopt(argc, argv, "r")) >= 0)
        if (c == 'r') o.remove_reads = true;
    if (optind + 1 >= argc) {
        fputs("Usage: samtools fixmate <in.nameSrt.bam> <out.nameSrt.bam>\n"
              "Options:\n"
              "       -r    remove unmapped reads and secondary alignments\n",
              stderr);
        return false;
    }
    o.in = argv[optind], o.out = argv[optind + 1];
    return true;
}

struct Rec {
    std::vector<uint8_t> b;      // block_size and the record's block_size bytes
    uint32_t word(size_t at) const
    {
        uint32_t v;
        memcpy(&v, &b[at], 4);
        return v;
    }
    void set(size_t at, uint32_t v) { memcpy(&b[at], &v, 4); }
    int32_t tid() const { return (int32_t)word(4); }
    int32_t pos() const { return (int32_t)word(8); }
    uint32_t l_qname() const { return b[12]; }
    uint32_t n_cigar() const { return word(16) & 0xffffu; }
    uint32_t flag() const { return word(16) >> 16; }
    void set_flag(uint32_t f) { set(16, (word(16) & 0xffffu) | f << 16); }
    void set_mate(int32_t mtid, int32_t mpos) { set(24, (uint32_t)mtid), set(28, (uint32_t)mpos); }
    void set_isize(uint32_t v) { set(32, v); }
    uint32_t cigar(uint32_t k) const
    {
        const size_t at = 36 + (size_t)l_qname() + 4 * (size_t)k;
        if (at + 4 > b.size()) throw Undefined{"a CIGAR runs past its record"};
        return word(at);
    }
    const char *name() const      // bam1_qname as a C string
    {
        if (b.size() <= 36 || !memchr(&b[36], 0, b.size() - 36)) throw Undefined{"a read name runs past its record"};
        return (const char *)&b[36];
    }
};

inline int cigar_type(uint32_t op) { return (int)(0x3C1A7u >> (op << 1) & 3u); }      // BAM_CIGAR_TYPE, 0 from op 9 up

// bam_calend (bam.c:17-41), with the backward walk of the B op
inline int32_t calend(const Rec &r)
{
    const int n = (int)r.n_cigar();
    uint32_t end = (uint32_t)r.pos();       // (int in the reference; unsigned here so that nothing overflows undefined)
    for (int k = 0; k < n; ++k) {
        const uint32_t c = r.cigar((uint32_t)k), op = c & 15u, len = c >> 4;
        if (op == 9u) {
            if (k == n - 1) break;
            int l;
            uint32_t u = 0, v = 0;
            for (l = k - 1; l >= 0; --l) {
                const uint32_t c1 = r.cigar((uint32_t)l), op1 = c1 & 15u, len1 = c1 >> 4;
                if (cigar_type(op1) & 1) {
                    if (u + len1 >= len) {
                        if (cigar_type(op1) & 2) v += len - u;
                        break;
                    }
                    u += len1;
                }
                if (cigar_type(op1) & 2) v += len1;
            }
            end = l < 0 ? (uint32_t)r.pos() : end - v;
        } else if (cigar_type(op) & 2) {
            end += len;
        }
    }
    return (int32_t)end;
}

inline void put_number(std::string &s, int32_t v)      // kputw
{
    char buf[16];
    int l = 0;
    uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    do buf[l++] = (char)('0' + mag % 10u), mag /= 10u;
    while (mag);
    if (v < 0) buf[l++] = '-';
    while (l) s.push_back(buf[--l]);
}

inline void put_side(std::string &s, const Rec &r)
{
    s.push_back(r.flag() & 0x40u ? '1' : '2');
    s.push_back(r.flag() & 0x10u ? 'R' : 'F');
    for (uint32_t k = 0; k < r.n_cigar(); ++k) {
        const uint32_t c = r.cigar(k), op = c & 15u;
        if (op > 10u) throw Undefined{"a CIGAR op above 10 in a CT field (the reference reads past BAM_CIGAR_STR)"};
        put_number(s, (int32_t)(c >> 4));
        s.push_back("MIDNSHP=XB"[op]);       // (op 10 is the string's NUL: the field ends there for every reader, its bytes go on)
    }
}

// bam_template_cigar(b1, b2): true when a CT field was appended
inline bool template_cigar(Rec &b1, Rec &b2, uint64_t *added)
{
    if (b1.tid() != b2.tid() || b1.tid() < 0) return false;
    Rec *lo = &b1, *hi = &b2;
    if (lo->pos() > hi->pos()) std::swap(lo, hi);
    std::string s;
    put_side(s, *lo);
    put_number(s, (int32_t)((uint32_t)hi->pos() - (uint32_t)calend(*lo)));
    s.push_back('T');
    put_side(s, *hi);
    const size_t was = lo->b.size();
    lo->b.insert(lo->b.end(), {'C', 'T', 'Z'});
    lo->b.insert(lo->b.end(), s.begin(), s.end());
    lo->b.push_back(0);
    lo->set(0, (uint32_t)(lo->b.size() - 4));
    *added += lo->b.size() - was;
    return true;
}

struct Counts {
    uint64_t n_records = 0, n_out = 0, n_pairs = 0, n_singletons = 0, n_tags = 0, bytes_added = 0;
};

// bam_mating_core behind the header: next(rec) reads a record (false at the end), write(rec) is bam_write1
template <class Next, class Write>
inline void mating_core(const std::vector<int32_t> &target_len, bool remove_reads, Next &&next, Write &&write, Counts &n)
{
    Rec b[2];
    int curr = 0;
    bool has_prev = false;
    int32_t pre_end = 0;
    auto out = [&](const Rec &r) { write(r), ++n.n_out; };
    while (next(b[curr])) {
        ++n.n_records;
        Rec &cur = b[curr], &pre = b[1 - curr];
        if (cur.tid() < 0) {
            if (!remove_reads) out(cur);
            continue;
        }
        const int32_t cur_end = calend(cur);
        if ((size_t)cur.tid() >= target_len.size()) throw Undefined{"a refID the header does not have"};
        if (cur_end > target_len[(size_t)cur.tid()]) cur.set_flag(cur.flag() | 0x4u);
        if (cur.flag() & 0x100u) {
            if (!remove_reads) out(cur);
            continue;
        }
        if (has_prev) {
            if (strcmp(cur.name(), pre.name()) == 0) {
                cur.set_mate(pre.tid(), pre.pos()), pre.set_mate(cur.tid(), cur.pos());
                if (pre.tid() == cur.tid() && !(cur.flag() & 0xcu) && !(pre.flag() & 0xcu)) {
                    const uint32_t cur5 = cur.flag() & 0x10u ? (uint32_t)cur_end : (uint32_t)cur.pos();
                    const uint32_t pre5 = pre.flag() & 0x10u ? (uint32_t)pre_end : (uint32_t)pre.pos();
                    cur.set_isize(pre5 - cur5), pre.set_isize(cur5 - pre5);
                } else {
                    cur.set_isize(0), pre.set_isize(0);
                }
                cur.set_flag(pre.flag() & 0x10u ? cur.flag() | 0x20u : cur.flag() & ~0x20u);
                pre.set_flag(cur.flag() & 0x10u ? pre.flag() | 0x20u : pre.flag() & ~0x20u);
                if (cur.flag() & 0x4u) pre.set_flag((pre.flag() | 0x8u) & ~0x2u);
                if (pre.flag() & 0x4u) cur.set_flag((cur.flag() | 0x8u) & ~0x2u);
                if (template_cigar(pre, cur, &n.bytes_added)) ++n.n_tags;
                out(pre), out(cur);
                ++n.n_pairs;
                has_prev = false;
            } else {
                pre.set_mate(-1, -1), pre.set_isize(0);
                if (pre.flag() & 0x1u) pre.set_flag((pre.flag() | 0x8u) & ~(0x20u | 0x2u));
                out(pre);
                ++n.n_singletons;
            }
        } else {
            has_prev = true;
        }
        curr = 1 - curr;
        pre_end = cur_end;
    }
    if (has_prev) out(b[1 - curr]);
}

// `samtools fixmate` behind its argument check.  Returns the status (0 as the reference; 2 where the reference's behaviour is
// undefined or it crashes: no output is left).
inline int fixmate_on_host(const Options &o)
{
    const bool from_stdin = strcmp(o.in, "-") == 0, to_stdout = strcmp(o.out, "-") == 0;
    FILE *f = fopen(from_stdin ? "/dev/stdin" : o.in, "rb");
    if (!f) {
        fprintf(stderr, "[hpn] bam_fixmate: %s: %s (the reference ends with a segmentation fault here)\n", o.in, strerror(errno));
        return 2;
    }
    const bool eof_marker = !from_stdin && bai::has_eof_marker(f);     // (recorded: the reference cannot seek in a pipe and says the marker is absent)
    bai::BgzfSeq z(f);
    bamsort::Header hdr;
    const int hr = bamsort::read_header(z, hdr);
    if (hr != 0) {
        fclose(f);
        fprintf(stderr, "[hpn] bam_fixmate: %s: outside the tool's domain\n", hr == -1 ? "the input is no BAM file" : "the header ends early");
        return 2;
    }
    if (!eof_marker) fputs("[bam_header_read] EOF marker is absent. The input is probably truncated.\n", stderr);
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), -1, head_blocks)) {
        fclose(f);
        fputs("[hpn] bam_fixmate: deflating the header failed\n", stderr);
        return 2;
    }
    BgzfWriter w(-1);
    if (!w.begin(to_stdout ? "/dev/stdout" : o.out, head_blocks)) {
        fclose(f);
        fprintf(stderr, "[hpn] bam_fixmate: %s: %s (the reference ends with a segmentation fault here)\n", o.out, strerror(errno));
        return 2;
    }
    auto emit = [&](const uint8_t *p, uint32_t n) { w.add(p, n, 0, false); };
    BgzfCutter<decltype(emit)> cut(emit);
    // a record as bam_read1 takes it (the loop ends without a word where one is cut short)
    auto next = [&](Rec &r) {
        int32_t block_len;
        if (z.read(&block_len, 4) != 4) return false;
        uint8_t core[32];
        if (z.read(core, 32) != 32) return false;
        const int64_t want = (int64_t)block_len - 32;
        if (want < 0) return false;
        r.b.resize(36);
        memcpy(&r.b[0], &block_len, 4), memcpy(&r.b[4], core, 32);
        for (int64_t have = 0; have < want;) {      // in pieces: a damaged size word does not allocate 2 GB
            const int64_t k = want - have < (1 << 20) ? want - have : (1 << 20);
            r.b.resize(36 + (size_t)(have + k));
            if (z.read(&r.b[36 + (size_t)have], k) != k) return false;
            have += k;
        }
        return true;
    };
    Counts n;
    try {
        mating_core(hdr.len, o.remove_reads, next, [&](const Rec &r) { cut.record(r.b.data(), r.b.size()); }, n);
    } catch (const Undefined &u) {
        fclose(f);
        fprintf(stderr, "[hpn] bam_fixmate: %s: the reference's behaviour is undefined here, nothing is written\n", u.what.c_str());
        w.abandon();
        if (!to_stdout) unlink(o.out);
        return 2;
    }
    fclose(f);
    cut.close();
    if (!w.finish()) {
        fprintf(stderr, "[hpn] bam_fixmate: writing %s failed\n", o.out);
        return 2;
    }
    return 0;
}

}  // namespace fixmate
}  // namespace hpn
