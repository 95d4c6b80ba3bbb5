// bam_merge_host.hpp -- samtools-0.1.19's `merge` on the host: the options, the usage text and the two early exits, the header
// rule with its messages, -h, and the sequential merger (the route of -n, -r and -h, of HPN_BAM_GPU=0 and the fallback of
// bin/bam_merge outside the device's domain).  (docs/kernels/bam_merge.md states the rules; tests/bammerge_ref.py is the same in
// Python, tests/golden/bammerge/ the recorded runs.)
//
// The reference keeps one record per input in a heap ordered by (uint64_t)refID << 32 | (uint32_t)(pos + 1) << 1 | strand, ties
// to the lower file number, and writes the top until the top's key is HEAP_EMPTY (all ones) -- which is also the key of a record
// with refID -1, reverse strand and pos -2 or 2^31 - 2: there the output ends early, with status 0.  It never checks that its
// inputs are sorted.  With -n the heap compares names (strnum_cmp, then flag & 0xc0) but still ends at a top whose coordinate
// key is HEAP_EMPTY.  The merger here is that heap over streaming readers: one record per input in memory.
//
// Where the reference's behaviour is undefined the tool says so and leaves with status 2: an input that is no BAM file or whose
// header ends early, an input that ends inside a record behind its first one (the reference writes the record before it again
// and again), -n with an input of no records or a read name without its end (it compares a null name), -r on a record whose aux
// fields lead outside it, a -h file with a header line without its end.  -R is not supported: status 2 before anything is opened.
// Nothing here needs a GPU: tests/bammerge_host_main.cpp builds this header alone.
#pragma once
#include <zlib.h>

#include <memory>

#include "bam_sort_host.hpp"

namespace hpn {
namespace bammerge {

struct Options {
    bool by_name = false, rg = false, uncomp = false, level1 = false, force = false;
    int level = -1, n_threads = 0;
    const char *headers = nullptr, *reg = nullptr, *out = nullptr;
    std::vector<const char *> in;
};

// bam_merge's own argument handling and what it does before it opens an input.  0: go on; else the status to leave with (the
// message has been printed): 1 fewer than three file arguments, or the output exists and -f is absent; 2 -R.
inline int parse_args(int argc, char *argv[], Options &o)
{
    int c;
    while ((c = getopt(argc, argv, "h:nru1R:f@:l:")) >= 0) {
        switch (c) {
        case 'r': o.rg = true; break;
        case 'f': o.force = true; break;
        case 'h': o.headers = optarg; break;
        case 'n': o.by_name = true; break;
        case '1': o.level1 = true; break;
        case 'u': o.uncomp = true; break;
        case 'R': o.reg = optarg; break;
        case 'l': o.level = atoi(optarg); break;
        case '@': o.n_threads = atoi(optarg); break;
        }
    }
    if (optind + 2 >= argc) {
        fputs("\nUsage:   samtools merge [-nr] [-h inh.sam] <out.bam> <in1.bam> <in2.bam> [...]\n\n"
              "Options: -n       sort by read names\n"
              "         -r       attach RG tag (inferred from file names)\n"
              "         -u       uncompressed BAM output\n"
              "         -f       overwrite the output BAM if exist\n"
              "         -1       compress level 1\n"
              "         -l INT   compression level, from 0 to 9 [-1]\n"
              "         -@ INT   number of BAM compression threads [0]\n"
              "         -R STR   merge file in the specified region STR [all]\n"
              "         -h FILE  copy the header in FILE to <out.bam> [in1.bam]\n\n"
              "Note: Samtools' merge does not reconstruct the @RG dictionary in the header. Users\n"
              "      must provide the correct header with -h, or uses Picard which properly maintains\n"
              "      the header dictionary in merging.\n\n",
              stderr);
        return 1;
    }
    if (o.reg) {
        fputs("bam_merge: -R (merging a region through the inputs' indices) is not supported\n", stderr);
        return 2;
    }
    o.out = argv[optind];
    for (int k = optind + 1; k < argc; ++k) o.in.push_back(argv[k]);
    if (!o.force && strcmp(o.out, "-") != 0) {
        FILE *fp = fopen(o.out, "rb");
        if (fp) {
            fclose(fp);
            fprintf(stderr, "[bam_merge] File '%s' exists. Please apply '-f' to overwrite. Abort.\n", o.out);
            return 1;
        }
    }
    return 0;
}

// The level the writer is opened with.  bam_merge_core2 works a mode string out of the options -- -u gives "w0", else -1 gives
// "w1", else -l INT ("w9" for 9 and more, plain "w" below 0) -- and then opens the output with the literal "w": in samtools-0.1.19
// -u, -1 and -l change no byte of the output (the recorded runs agree), and neither do they here.  -u only keeps the reference
// from starting its compression threads.
inline int level_of(const Options &) { return -1; }
inline std::string output_path(const Options &o) { return strcmp(o.out, "-") ? o.out : "/dev/stdout"; }

// the heap's key: the low word is cut to 32 bits before it meets the high word
inline uint64_t key_of(int32_t tid, int32_t pos, uint32_t flag)
{
    return ((uint64_t)(int64_t)tid << 32) | (uint32_t)(((uint32_t)pos + 1u) << 1) | ((flag >> 4) & 1u);
}
constexpr uint64_t kHeapEmpty = ~0ull;

// -h FILE as sam_header_read takes it: the text is the file's leading lines that begin with '@'; the @SQ lines' SN values are the
// names the binary list is checked against.  0 read, -1 the file cannot be opened (errno says why), -2 a line without its end
inline int read_sam_header(const char *path, std::string &text, std::vector<std::string> &sq)
{
    gzFile g = gzopen(path, "rb");
    if (!g) return -1;
    std::string all;
    char buf[1 << 16];
    int got;
    while ((got = gzread(g, buf, sizeof buf)) > 0) all.append(buf, (size_t)got);
    gzclose(g);
    text.clear(), sq.clear();
    for (size_t at = 0; at < all.size() && all[at] == '@';) {
        const size_t e = all.find('\n', at);
        if (e == std::string::npos) return -2;
        const std::string line = all.substr(at, e - at);
        text += line, text += '\n';
        if (line.compare(0, 4, "@SQ\t") == 0) {
            size_t p = 3;
            while (p != std::string::npos && p < line.size()) {
                const size_t q = line.find('\t', p + 1);
                if (line.compare(p + 1, 3, "SN:") == 0) {
                    sq.push_back(line.substr(p + 4, q == std::string::npos ? q : q - p - 4));
                    break;
                }
                p = q;
            }
        }
        at = e + 1;
    }
    return 0;
}

// Everything bam_merge_core2 does before it reads a record: -h FILE read, every input opened and its header read in argument
// order, the target lists compared over their common front and the longest one kept, -h's checks and its text swapped in.
// What the reference would have printed goes to `err`.  0: `out` is the output's header; 1: the reference leaves with status 1;
// 2: outside the tool's domain (the reason is in `err`).
inline int prepare(const Options &o, bamsort::Header &out, std::string &err)
{
    std::string h_text;
    std::vector<std::string> h_sq;
    if (o.headers) {
        const int r = read_sam_header(o.headers, h_text, h_sq);
        if (r == -1) {
            err += std::string("[bam_merge_core] cannot open '") + o.headers + "': " + strerror(errno) + "\n";
            return 1;
        }
        if (r == -2) {
            err += std::string("bam_merge: ") + o.headers + ": a header line without its end: outside the tool's domain\n";
            return 2;
        }
    }
    for (size_t i = 0; i < o.in.size(); ++i) {
        FILE *f = fopen(o.in[i], "rb");
        if (!f) {
            err += std::string("open: ") + strerror(errno) + "\n[bam_merge_core] fail to open file " + o.in[i] + "\n";
            return 1;
        }
        if (!bai::has_eof_marker(f)) err += "[bam_header_read] EOF marker is absent. The input is probably truncated.\n";
        bai::BgzfSeq z(f);
        bamsort::Header hin;
        const int hr = bamsort::read_header(z, hin);
        fclose(f);
        if (hr != 0) {
            err += std::string("bam_merge: ") + o.in[i] + (hr == -1 ? ": no BAM file" : ": the header ends early") + ": outside the tool's domain\n";
            return 2;
        }
        if (i == 0) {
            out = hin;
            continue;
        }
        const size_t common = std::min(out.name.size(), hin.name.size());
        for (size_t j = 0; j < common; ++j)
            if (out.name[j] != hin.name[j]) {
                err += "[bam_merge_core] different target sequence name: '" + out.name[j] + "' != '" + hin.name[j] + "' in file '" + o.in[i] + "'\n";
                return 1;
            }
        if (hin.name.size() > out.name.size()) out.name.swap(hin.name), out.len.swap(hin.len);      // swap_header_targets
    }
    if (o.headers) {
        if (!h_sq.empty()) {
            if (h_sq.size() != out.name.size()) {
                err += std::string("[bam_merge_core] number of @SQ headers in '") + o.headers + "' differs from number of target sequences\n";
                return 1;
            }
            for (size_t j = 0; j < out.name.size(); ++j)
                if (out.name[j] != h_sq[j]) {
                    err += "[bam_merge_core] @SQ header '" + h_sq[j] + "' in '" + o.headers + "' differs from target sequence\n";
                    return 1;
                }
        }
        out.text = h_text;
    }
    return 0;
}

// -r: the name of input i's read group, its file name without the directories and without a final ".bam"
inline std::string rg_name(const char *fn)
{
    std::string s(fn);
    if (s.size() > 4 && s.compare(s.size() - 4, 4, ".bam") == 0) s.resize(s.size() - 4);
    const size_t slash = s.rfind('/');
    return slash == std::string::npos ? s : s.substr(slash + 1);
}

// -r on one record (4 + block_size bytes): bam_aux_get("RG") with bam_aux_del, then bam_aux_append("RG", 'Z', name).  The walk
// is bam_aux.c's: the tag's two bytes, the type (upper-cased: Z and H run to their NUL, B has a subtype and a count, C and A take
// 1 byte, S 2, I and F 4, anything else 0).  false: the fields lead outside the record.
inline bool rg_edit(std::vector<uint8_t> &r, const std::string &name)
{
    const size_t l_qname = r[12], n_cigar = (size_t)r[16] | (size_t)r[17] << 8;
    int32_t l_qseq;
    memcpy(&l_qseq, &r[20], 4);
    if (l_qseq < 0) return false;
    const size_t aux = 36 + l_qname + 4 * n_cigar + ((size_t)l_qseq + 1) / 2 + (size_t)l_qseq, end = r.size();
    if (aux > end) return false;
    auto width = [](int t) { return t == 'C' || t == 'A' ? 1u : t == 'S' ? 2u : t == 'I' || t == 'F' ? 4u : 0u; };
    auto skip = [&](size_t &s) {      // s at the type byte -> behind the value; false: outside
        if (s >= end) return false;
        const int type = toupper(r[s++]);
        if (type == 'Z' || type == 'H') {
            while (s < end && r[s]) ++s;
            if (s >= end) return false;
            ++s;
        } else if (type == 'B') {
            if (s + 5 > end) return false;
            int32_t cnt;
            memcpy(&cnt, &r[s + 1], 4);
            const int sub = r[s];
            const unsigned w = sub == 'C' || sub == 'c' || sub == 'A' ? 1u : sub == 'S' || sub == 's' ? 2u : sub == 'I' || sub == 'i' || sub == 'f' || sub == 'F' ? 4u : 0u;
            if (cnt < 0 || (uint64_t)w * (uint64_t)cnt > end) return false;
            s += 5 + (size_t)w * (size_t)cnt;
        } else {
            s += width(type);
        }
        return s <= end;
    };
    for (size_t s = aux; s < end;) {
        if (s + 2 > end) return false;
        const bool hit = r[s] == 'R' && r[s + 1] == 'G';
        const size_t tag = s;
        s += 2;
        if (!skip(s)) return false;
        if (hit) {
            r.erase(r.begin() + (ptrdiff_t)tag, r.begin() + (ptrdiff_t)s);
            break;
        }
    }
    r.push_back('R'), r.push_back('G'), r.push_back('Z');
    r.insert(r.end(), name.begin(), name.end());
    r.push_back(0);
    const uint32_t bs = (uint32_t)r.size() - 4u;
    memcpy(&r[0], &bs, 4);
    return true;
}

struct Reader {
    FILE *f = nullptr;
    std::unique_ptr<bai::BgzfSeq> z;
    std::vector<uint8_t> rec;      // the record at hand, 4 + block_size bytes
    ~Reader()
    {
        if (f) fclose(f);
    }
    // 0 a record, -1 the end, below -1 the file ends inside a record
    int next()
    {
        int32_t block_len;
        const int64_t got = z->read(&block_len, 4);
        if (got != 4) return got == 0 ? -1 : -2;
        rec.resize(36);
        memcpy(&rec[0], &block_len, 4);
        if (z->read(&rec[4], 32) != 32) return -3;
        const int64_t want = (int64_t)block_len - 32;
        if (want < 0) return -4;
        for (int64_t have = 0; have < want;) {      // in pieces: a damaged size word does not allocate 2 GB
            const int64_t k = want - have < (1 << 20) ? want - have : (1 << 20);
            rec.resize(36 + (size_t)(have + k));
            if (z->read(&rec[36 + (size_t)have], k) != k) return -4;
            have += k;
        }
        return 0;
    }
};

// `samtools merge` behind parse_args.  Returns the status (0, 1; 2 where the reference's behaviour is undefined).
inline int merge_on_host(const Options &o)
{
    bamsort::Header hdr;
    std::string err;
    const int ps = prepare(o, hdr, err);
    fputs(err.c_str(), stderr);
    if (ps != 0) return ps;
    const size_t n = o.in.size();
    std::vector<Reader> in(n);
    std::vector<std::string> rg(n);
    for (size_t i = 0; i < n; ++i) {
        bamsort::Header skip;
        in[i].f = fopen(o.in[i], "rb");
        if (in[i].f) in[i].z.reset(new bai::BgzfSeq(in[i].f));
        if (!in[i].f || bamsort::read_header(*in[i].z, skip) != 0) {
            fprintf(stderr, "bam_merge: %s changed while it was read\n", o.in[i]);
            return 2;
        }
        if (o.rg) rg[i] = rg_name(o.in[i]);
    }
    struct Entry {
        int i;
        uint64_t pos, idx;
        bool live;      // the reference's b != 0
    };
    uint64_t idx = 0;
    std::vector<Entry> heap(n);
    auto name_of = [&](const Entry &e) { return (const char *)&in[(size_t)e.i].rec[36]; };
    auto flag_of = [&](const Entry &e) { return (uint32_t)in[(size_t)e.i].rec[18] | (uint32_t)in[(size_t)e.i].rec[19] << 8; };
    auto keyed = [&](Entry &e) {      // false: -n and a name without its end
        const std::vector<uint8_t> &r = in[(size_t)e.i].rec;
        int32_t tid, pos;
        memcpy(&tid, &r[4], 4), memcpy(&pos, &r[8], 4);
        e.pos = key_of(tid, pos, flag_of(e)), e.idx = idx++;
        return !o.by_name || memchr(&r[36], 0, r.size() - 36) != nullptr;
    };
    const char *no_name = "bam_merge: a read name without its end: outside the tool's domain\n";
    for (size_t i = 0; i < n; ++i) {
        Entry &e = heap[i];
        e.i = (int)i, e.idx = 0, e.live = true;
        if (in[i].next() == 0) {
            if (!keyed(e)) return fputs(no_name, stderr), 2;
        } else {
            e.pos = kHeapEmpty;      // (the end, or a first record that ends early: the reference takes both as the end)
            if (o.by_name) {
                fprintf(stderr, "bam_merge: -n and %s holds no record: outside the tool's domain\n", o.in[i]);
                return 2;
            }
        }
    }
    const int level = level_of(o);
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), level, head_blocks)) {
        fputs("bam_merge: deflating the header failed\n", stderr);
        return 2;
    }
    const std::string path = output_path(o);
    BgzfWriter w(level);
    if (!w.begin(path.c_str(), head_blocks)) {
        fputs("[bam_merge_core2] fail to create the output file.\n", stderr);
        return 1;
    }
    auto heap_lt = [&](const Entry &a, const Entry &b) {
        if (o.by_name) {
            if (!a.live || !b.live) return !a.live;
            const int t = bamsort::strnum_cmp(name_of(a), name_of(b));
            return t > 0 || (t == 0 && (flag_of(a) & 0xc0u) > (flag_of(b) & 0xc0u));
        }
        return a.pos > b.pos || (a.pos == b.pos && (a.i > b.i || (a.i == b.i && a.idx > b.idx)));
    };
    auto adjust = [&](size_t i) {      // ks_heapadjust: the entry at i sinks below its smaller child
        size_t k = i;
        const Entry tmp = heap[i];
        while ((k = (k << 1) + 1) < n) {
            if (k != n - 1 && heap_lt(heap[k], heap[k + 1])) ++k;
            if (heap_lt(heap[k], tmp)) break;
            heap[i] = heap[k], i = k;
        }
        heap[i] = tmp;
    };
    for (size_t i = n >> 1; i-- > 0;) adjust(i);
    auto emit = [&](const uint8_t *p, uint32_t m) { w.add(p, m, 0, false); };
    BgzfCutter<decltype(emit)> cut(emit);
    int status = 0;
    while (heap[0].pos != kHeapEmpty) {
        Reader &r = in[(size_t)heap[0].i];
        if (o.rg && !rg_edit(r.rec, rg[(size_t)heap[0].i])) {
            fputs("bam_merge: -r and a record whose aux fields lead outside it: outside the tool's domain\n", stderr);
            status = 2;
            break;
        }
        cut.record(r.rec.data(), r.rec.size());
        const int j = r.next();
        if (j == 0) {
            if (!keyed(heap[0])) {
                fputs(no_name, stderr);
                status = 2;
                break;
            }
        } else if (j == -1) {
            heap[0].pos = kHeapEmpty, heap[0].live = false;
        } else {      // the reference says this and writes the record before it again, without end
            fprintf(stderr, "[bam_merge_core] '%s' is truncated. Continue anyway.\n", o.in[(size_t)heap[0].i]);
            fprintf(stderr, "bam_merge: %s ends inside a record: outside the tool's domain\n", o.in[(size_t)heap[0].i]);
            status = 2;
            break;
        }
        adjust(0);
    }
    cut.close();
    if (!w.finish()) {
        fprintf(stderr, "bam_merge: writing %s failed\n", path.c_str());
        return 2;
    }
    return status;
}

}  // namespace bammerge
}  // namespace hpn
