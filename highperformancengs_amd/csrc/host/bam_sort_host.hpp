// bam_sort_host.hpp -- samtools-0.1.19's `sort` on the host: the options, the header's SO field, the reference's chunk
// accounting, and the sequential sorter (the route of -n, of HPN_BAM_GPU=0 and the fallback of bin/bam_sort outside the device's
// domain).  (docs/kernels/bam_sort.md states the rules; tests/bamsort_ref.py is the same in Python, tests/golden/bamsort/ the
// recorded runs.)
//
// The reference reads records until the memory it counts for them reaches max_mem, sorts that chunk (with -@ N: in N parts) into
// temporary files, and merges the files through a heap.  The order that comes out depends on the chunks only where the sort's key
// and the heap's key disagree -- pos below -1 or above 2^30 - 2 -- or, by name, where the heap meets equal names; the sorter here
// follows the chunking everywhere, in memory, and writes no temporary file.  What always depends on the chunking: the
// "merging from N files" message and the level of the output, which the merge step opens with mode "w" whatever -l says.
// Nothing here needs a GPU: tests/bamsort_host_main.cpp builds this header alone.
#pragma once
#include <ctype.h>
#include <getopt.h>
#include <stdlib.h>

#include "bai_build.hpp"
#include "bgzf_writer.hpp"

namespace hpn {
namespace bamsort {

struct Options {
    bool by_name = false, full_path = false, to_stdout = false;
    int level = -1, n_threads = 0;
    size_t max_mem = (size_t)768 << 20;
    const char *in = nullptr, *prefix = nullptr;
};

// bam_sort's own argument handling; false: fewer than two arguments remain (the usage text has been printed, status 1)
inline bool parse_args(int argc, char *argv[], Options &o)
{
    int c;
    while ((c = getopt(argc, argv, "fnom:@:l:")) >= 0) {
        switch (c) {
        case 'f': o.full_path = true; break;
        case 'o': o.to_stdout = true; break;
        case 'n': o.by_name = true; break;
        case 'm': {
            char *q;
            o.max_mem = (size_t)strtol(optarg, &q, 0);
            if (*q == 'k' || *q == 'K') o.max_mem <<= 10;
            else if (*q == 'm' || *q == 'M') o.max_mem <<= 20;
            else if (*q == 'g' || *q == 'G') o.max_mem <<= 30;
            break;
        }
        case '@': o.n_threads = atoi(optarg); break;
        case 'l': o.level = atoi(optarg); break;
        }
    }
    if (optind + 2 > argc) {
        fputs("\nUsage:   samtools sort [options] <in.bam> <out.prefix>\n\n"
              "Options: -n        sort by read name\n"
              "         -f        use <out.prefix> as full file name instead of prefix\n"
              "         -o        final output to stdout\n"
              "         -l INT    compression level, from 0 to 9 [-1]\n"
              "         -@ INT    number of sorting and compression threads [1]\n"
              "         -m INT    max memory per thread; suffix K/M/G recognized [768M]\n\n",
              stderr);
        return false;
    }
    o.in = argv[optind], o.prefix = argv[optind + 1];
    return true;
}

inline int threads_of(const Options &o) { return o.n_threads < 2 ? 1 : o.n_threads; }
inline size_t max_mem_of(const Options &o) { return o.max_mem * (size_t)threads_of(o); }
inline std::string output_path(const Options &o) { return o.to_stdout ? "/dev/stdout" : std::string(o.prefix) + (o.full_path ? "" : ".bam"); }
// the level a writer is opened with: mode "w" + the digit for 0 .. 9 (above 9: 9), plain "w" -- the default -- below 0
inline int level_of(int level) { return level < 0 ? -1 : level < 9 ? level : 9; }

// change_SO: the text of the header with SO:<so> in its @HD line.  An @HD line is the text's start "@HD" up to the first line
// end; its SO value is compared over the rest of the line only as far as that rest reaches (so a value that is a prefix of <so>
// at the end of the line stays, and a value followed by another field is rewritten); without @HD a line of VN:1.3 goes in front;
// an @HD line without its end leaves the text alone.
inline void change_so(std::string &text, const char *so)
{
    const std::string t(text.c_str());      // (what the C string functions see)
    const size_t none = std::string::npos;
    size_t beg = none, end = none;
    if (text.size() > 3 && t.compare(0, 3, "@HD") == 0) {
        const size_t p = t.find('\n');
        if (p == none) return;
        const size_t q = t.substr(0, p).find("\tSO:");
        if (q != none) {
            if (strncmp(t.c_str() + q + 4, so, p - q - 4) == 0) return;
            beg = q;
            size_t e = q + 4;
            while (t[e] != '\n' && t[e] != '\t') ++e;
            end = e;
        } else {
            beg = end = p;
        }
    }
    if (beg == none) text = std::string("@HD\tVN:1.3\tSO:") + so + "\n" + text;
    else text = text.substr(0, beg) + "\tSO:" + so + text.substr(end);
}

struct Header {
    std::string text;
    std::vector<std::string> name;
    std::vector<int32_t> len;
    // as bam_header_write writes it: a name's length is its C string's + 1
    std::vector<uint8_t> bytes() const
    {
        std::vector<uint8_t> out;
        auto put = [&](const void *p, size_t n) { out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + n); };
        const int32_t l_text = (int32_t)text.size(), n_ref = (int32_t)name.size();
        put("BAM\1", 4), put(&l_text, 4), put(text.data(), text.size()), put(&n_ref, 4);
        for (int32_t t = 0; t < n_ref; ++t) {
            const int32_t l_name = (int32_t)name[(size_t)t].size() + 1;
            put(&l_name, 4), put(name[(size_t)t].c_str(), (size_t)l_name), put(&len[(size_t)t], 4);
        }
        return out;
    }
};

// 0 read, -1 no BAM magic, -2 the header ends early
inline int read_header(bai::BgzfSeq &z, Header &h)
{
    char magic[4];
    if (z.read(magic, 4) != 4 || memcmp(magic, "BAM\1", 4) != 0) return -1;
    int32_t l_text, n_ref;
    if (z.read(&l_text, 4) != 4 || l_text < 0) return -2;
    h.text.resize((size_t)l_text);
    if (l_text && z.read(&h.text[0], l_text) != l_text) return -2;
    if (z.read(&n_ref, 4) != 4 || n_ref < 0) return -2;
    for (int32_t t = 0; t < n_ref; ++t) {
        int32_t l_name, l_ref;
        if (z.read(&l_name, 4) != 4 || l_name < 0) return -2;
        std::string nm((size_t)l_name, '\0');
        if (l_name && z.read(&nm[0], l_name) != l_name) return -2;
        if (z.read(&l_ref, 4) != 4) return -2;
        h.name.emplace_back(nm.c_str());
        h.len.push_back(l_ref);
    }
    return 0;
}

inline uint32_t roundup32(uint32_t x)      // kroundup32: the next power of two, 0 for 0 and above 2^31
{
    --x;
    x |= x >> 1, x |= x >> 2, x |= x >> 4, x |= x >> 8, x |= x >> 16;
    return ++x;
}

// The reference's temporary files over the records' sizes (4 + block_size each), as bam_sort_core_ext counts them: slot k of
// its buffer keeps its capacity from chunk to chunk -- it grows to the round-up of a longer record and shrinks to it when the
// record is shorter than a quarter --, a record costs 56 + capacity + 16, a chunk closes when the sum reaches max_mem and becomes
// n_threads files if it holds 64 records per thread, else one; once a chunk has closed the rest, even if empty, is one more.
// Sorting a file's records moves the slots with them: slot j of the next chunk has the capacity of the record sorted to place j,
// so the count depends on the order too.  less(a, b): record a sorts in front of record b (ordinals; ties keep their order).
// parts: every file's record count, in file order (empty: the reference sorts in one block); files: the records' ordinals, file
// after file, each file in its sorted order.
template <class Less>
inline void plan_chunks(const uint32_t *sizes, uint64_t n, size_t max_mem, int n_threads, Less less, std::vector<uint64_t> &parts,
                        std::vector<uint32_t> &files)
{
    parts.clear(), files.clear();
    std::vector<int32_t> cap, moved;
    size_t mem = 0;
    uint64_t k = 0, start = 0;
    auto close_chunk = [&](uint64_t count) {
        int nt = n_threads < 1 ? 1 : n_threads;
        if (count < (uint64_t)nt * 64) nt = 1;
        uint64_t rest = count, at = 0;
        for (int i = 0; i < nt; ++i) {
            const uint64_t len = rest / (uint64_t)(nt - i);
            const size_t f0 = files.size();
            for (uint64_t j = 0; j < len; ++j) files.push_back((uint32_t)(start + at + j));
            std::stable_sort(files.begin() + (ptrdiff_t)f0, files.end(), less);
            moved.resize((size_t)len);
            for (uint64_t j = 0; j < len; ++j) moved[(size_t)j] = cap[(size_t)(files[f0 + (size_t)j] - start)];
            std::copy(moved.begin(), moved.end(), cap.begin() + (ptrdiff_t)at);
            parts.push_back(len);
            rest -= len, at += len;
        }
    };
    for (uint64_t r = 0; r < n; ++r) {
        const int32_t data_len = (int32_t)(sizes[r] - 36u);
        if (k == cap.size()) cap.push_back(0);
        int32_t &m = cap[(size_t)k];
        if (m < data_len) m = (int32_t)roundup32((uint32_t)data_len);
        if (data_len < m >> 2) m = (int32_t)roundup32((uint32_t)data_len);
        mem += (size_t)56 + (size_t)(int64_t)m + 16;
        ++k;
        if (mem >= max_mem) close_chunk(k), mem = 0, k = 0, start = r + 1;
    }
    if (!parts.empty()) close_chunk(k);
}

// strnum_cmp: names compared piece by piece, runs of digits as numbers (leading zeros passed over, the longer run larger, equal
// values with different zero padding: the more padded one first), everything else as bytes
inline int strnum_cmp(const char *a_, const char *b_)
{
    const unsigned char *a = (const unsigned char *)a_, *b = (const unsigned char *)b_, *pa = a, *pb = b;
    while (*pa && *pb) {
        if (isdigit(*pa) && isdigit(*pb)) {
            while (*pa == '0') ++pa;
            while (*pb == '0') ++pb;
            while (isdigit(*pa) && isdigit(*pb) && *pa == *pb) ++pa, ++pb;
            if (isdigit(*pa) && isdigit(*pb)) {
                int i = 0;
                while (isdigit(pa[i]) && isdigit(pb[i])) ++i;
                return isdigit(pa[i]) ? 1 : isdigit(pb[i]) ? -1 : (int)*pa - (int)*pb;
            }
            if (isdigit(*pa)) return 1;
            if (isdigit(*pb)) return -1;
            if (pa - a != pb - b) return pa - a < pb - b ? 1 : -1;
        } else {
            if (*pa != *pb) return (int)*pa - (int)*pb;
            ++pa, ++pb;
        }
    }
    return *pa ? 1 : *pb ? -1 : 0;
}

struct Rec {
    uint64_t at;            // where its 4 + block_size bytes start in the buffer
    uint32_t size, flag;
    uint64_t lt_key, heap_key;
};

// the two keys: bam1_lt's, where (pos + 1) << 1 is a signed 32-bit value that is sign-extended into the high word, and the merge
// heap's, where it is cut to 32 bits
inline void keys_of(int32_t tid, int32_t pos, uint32_t flag, uint64_t &lt_key, uint64_t &heap_key)
{
    const uint32_t low = ((uint32_t)pos + 1u) << 1, strand = (flag >> 4) & 1u;
    lt_key = ((uint64_t)(int64_t)tid << 32) | (uint64_t)(int64_t)(int32_t)low | strand;
    heap_key = ((uint64_t)(int64_t)tid << 32) | low | strand;
}

// `samtools sort` behind its argument check.  Returns the status (0; 2 where the reference's behaviour is undefined).
inline int sort_on_host(const Options &o)
{
    FILE *f = fopen(strcmp(o.in, "-") ? o.in : "/dev/stdin", "rb");
    if (!f) {
        fprintf(stderr, "open: %s\n", strerror(errno));
        fprintf(stderr, "[bam_sort_core] fail to open file %s\n", o.in);
        return 0;
    }
    if (!bai::has_eof_marker(f)) fputs("[bam_header_read] EOF marker is absent. The input is probably truncated.\n", stderr);
    bai::BgzfSeq z(f);
    Header hdr;
    const int hr = read_header(z, hdr);
    if (hr != 0) {
        fclose(f);
        fprintf(stderr, "bam_sort: %s: outside the tool's domain\n", hr == -1 ? "the input is no BAM file" : "the header ends early");
        return 2;
    }
    change_so(hdr.text, o.by_name ? "queryname" : "coordinate");
    // every record, as bam_read1 takes them
    std::vector<uint8_t> buf;
    std::vector<Rec> recs;
    std::vector<uint32_t> sizes;
    int64_t status;
    for (;;) {
        int32_t block_len;
        const int64_t got = z.read(&block_len, 4);
        if (got != 4) {
            status = got == 0 ? -1 : -2;
            break;
        }
        uint32_t x[8];
        if (z.read(x, 32) != 32) {
            status = -3;
            break;
        }
        const int64_t want = (int64_t)block_len - 32;
        if (want < 0) {
            status = -4;
            break;
        }
        const size_t at = buf.size();
        buf.resize(at + 36);
        memcpy(&buf[at], &block_len, 4), memcpy(&buf[at + 4], x, 32);
        bool whole = true;
        for (int64_t have = 0; have < want && whole;) {      // in pieces: a damaged size word does not allocate 2 GB
            const int64_t k = want - have < (1 << 20) ? want - have : (1 << 20);
            buf.resize(at + 36 + (size_t)(have + k));
            whole = z.read(&buf[at + 36 + (size_t)have], k) == k;
            have += k;
        }
        if (!whole) {
            buf.resize(at);
            status = -4;
            break;
        }
        Rec r;
        r.at = at, r.size = (uint32_t)block_len + 4u, r.flag = x[3] >> 16;
        keys_of((int32_t)x[0], (int32_t)x[1], r.flag, r.lt_key, r.heap_key);
        recs.push_back(r), sizes.push_back(r.size);
    }
    fclose(f);
    if (status != -1) fputs("[bam_sort_core] truncated file. Continue anyway.\n", stderr);
    if (o.by_name)
        for (const Rec &r : recs)
            if (!memchr(&buf[r.at + 36], 0, r.size - 36)) {
                fputs("bam_sort: a read name without its end: outside the tool's domain\n", stderr);
                return 2;
            }

    auto name_of = [&](const Rec &r) { return (const char *)&buf[r.at + 36]; };
    auto lt = [&](const Rec &a, const Rec &b) {
        if (!o.by_name) return a.lt_key < b.lt_key;
        const int t = strnum_cmp(name_of(a), name_of(b));
        return t < 0 || (t == 0 && (a.flag & 0xc0u) < (b.flag & 0xc0u));
    };
    std::vector<uint64_t> parts;
    std::vector<uint32_t> files;
    plan_chunks(sizes.data(), sizes.size(), max_mem_of(o), threads_of(o), [&](uint32_t a, uint32_t b) { return lt(recs[a], recs[b]); }, parts, files);
    std::vector<uint32_t> order;      // the output: indices into recs
    int level = level_of(o.level);
    if (parts.empty()) {
        order.resize(recs.size());
        for (size_t k = 0; k < recs.size(); ++k) order[k] = (uint32_t)k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lt(recs[a], recs[b]); });
    } else {
        // every file sorted by itself, then the heap of the merge: ks_heapmake / ks_heapadjust over one entry per file
        std::vector<size_t> from(parts.size() + 1, 0);
        for (size_t p = 0; p < parts.size(); ++p) from[p + 1] = from[p] + (size_t)parts[p];
        fprintf(stderr, "[bam_sort_core] merging from %d files...\n", (int)parts.size());
        level = -1;
        struct Entry {
            int i;
            uint64_t pos, idx;
            int64_t rec;      // -1: the file is used up
        };
        const uint64_t kEmpty = ~0ull;
        uint64_t idx = 0;
        std::vector<size_t> next(from.begin(), from.end() - 1);
        std::vector<Entry> heap(parts.size());
        auto refill = [&](Entry &e) {
            const size_t p = (size_t)e.i;
            if (next[p] < from[p + 1]) e.rec = (int64_t)files[next[p]++], e.pos = recs[(size_t)e.rec].heap_key, e.idx = idx++;
            else e.rec = -1, e.pos = kEmpty;
        };
        auto heap_lt = [&](const Entry &a, const Entry &b) {
            if (o.by_name) {
                if (a.rec < 0 || b.rec < 0) return a.rec < 0;
                const Rec &ra = recs[(size_t)a.rec], &rb = recs[(size_t)b.rec];
                const int t = strnum_cmp(name_of(ra), name_of(rb));
                return t > 0 || (t == 0 && (ra.flag & 0xc0u) > (rb.flag & 0xc0u));
            }
            return a.pos > b.pos || (a.pos == b.pos && (a.i > b.i || (a.i == b.i && a.idx > b.idx)));
        };
        auto adjust = [&](size_t i, size_t n) {      // the entry at i sinks below its smaller child
            size_t k = i;
            const Entry tmp = heap[i];
            while ((k = (k << 1) + 1) < n) {
                if (k != n - 1 && heap_lt(heap[k], heap[k + 1])) ++k;
                if (heap_lt(heap[k], tmp)) break;
                heap[i] = heap[k], i = k;
            }
            heap[i] = tmp;
        };
        for (size_t p = 0; p < parts.size(); ++p) heap[p].i = (int)p, refill(heap[p]);
        const size_t n = heap.size();
        for (size_t i = n >> 1; i-- > 0;) adjust(i, n);
        while (heap[0].pos != kEmpty) {
            order.push_back((uint32_t)heap[0].rec);
            refill(heap[0]);
            adjust(0, n);
        }
    }

    const std::string path = output_path(o);
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), level, head_blocks)) {
        fputs("bam_sort: deflating the header failed\n", stderr);
        return 2;
    }
    BgzfWriter w(level);
    if (!w.begin(path.c_str(), head_blocks)) {
        if (!parts.empty()) fputs("[bam_merge_core2] fail to create the output file.\n", stderr);
        return 0;
    }
    auto emit = [&](const uint8_t *p, uint32_t n) { w.add(p, n, 0, false); };
    BgzfCutter<decltype(emit)> cut(emit);
    for (uint32_t k : order) cut.record(&buf[recs[k].at], recs[k].size);
    cut.close();
    if (!w.finish()) {
        fprintf(stderr, "bam_sort: writing %s failed\n", path.c_str());
        return 2;
    }
    return 0;
}

}  // namespace bamsort
}  // namespace hpn
