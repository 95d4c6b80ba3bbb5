// bam_rmdup_host.hpp -- samtools-0.1.19's `rmdup` on the host: the options, the library of a record (the header's @RG lines as
// sam_header_parse2 and sam_header2tbl read them, the RG tag as bam_aux_get finds it), and both cores restated sequentially --
// bam_rmdup_core with its best_hash (cleared at a target change, or at a pos change once it holds 0x40000 keys), its stack and its
// set of names; bam_rmdupse_core with its queue on recycled list nodes (flushed at a target change or beyond 0x100000 elements) --
// and the library lines in khash's iteration order.  The route of -s / -S, of HPN_BAM_GPU=0 and the fallback of bin/bam_rmdup
// outside the device's domain.  (docs/kernels/bam_rmdup.md states the rules; tests/rmdup_ref.py is the same in Python,
// tests/golden/rmdup/ the recorded runs.)
//
// Where the reference would read memory that is not its own -- a hit on a best_hash key whose record has been written and
// freed (only unsorted input does that), an aux walk or a name past its record, a refID the header does not have -- Undefined is
// thrown: the tool says so under [hpn], leaves with status 2 and no output.  Nothing here needs a GPU:
// tests/rmdup_host_main.cpp builds this header alone.
#pragma once
#include <map>
#include <unordered_map>
#include <unordered_set>

#include "bam_sort_host.hpp"

namespace hpn {
namespace rmdup {

struct Options {
    bool se = false, force_se = false;
    const char *in = nullptr, *out = nullptr;
};

struct Undefined {
    std::string what;
};

// bam_rmdup's own argument handling; false: fewer than two arguments remain (the usage text has been printed, status 1)
inline bool parse_args(int argc, char *argv[], Options &o)
{
    int c;
    while ((c = getopt(argc, argv, "sS")) >= 0) {
        switch (c) {
        case 's': o.se = true; break;
        case 'S': o.force_se = o.se = true; break;
        }
    }
    if (optind + 2 > argc) {
        fputs("\nUsage:  samtools rmdup [-sS] <input.srt.bam> <output.bam>\n\n"
              "Option: -s    rmdup for SE reads\n"
              "        -S    treat PE reads as SE in rmdup (force -s)\n\n",
              stderr);
        return false;
    }
    o.in = argv[optind], o.out = argv[optind + 1];
    return true;
}

// ---- a record's fields ----

struct Rec {
    const uint8_t *b;      // its 4 + block_size bytes
    uint32_t size;
    int32_t tid, pos, l_qseq, mtid, isize;
    uint32_t l_qname, n_cigar, flag;
    explicit Rec(const uint8_t *p = nullptr, uint32_t n = 0) : b(p), size(n)
    {
        if (!p) return;
        uint32_t x[8];
        memcpy(x, p + 4, 32);
        tid = (int32_t)x[0], pos = (int32_t)x[1], l_qname = x[2] & 0xff, n_cigar = x[3] & 0xffff, flag = x[3] >> 16;
        l_qseq = (int32_t)x[4], mtid = (int32_t)x[5], isize = (int32_t)x[7];
    }
    std::string name() const      // bam1_qname as a C string
    {
        const void *e = memchr(b + 36, 0, size - 36);
        if (!e) throw Undefined{"a read name runs past its record"};
        return std::string((const char *)b + 36, (const char *)e);
    }
    int64_t sum_qual() const
    {
        if (l_qseq < 0) return 0;
        const uint64_t at = 36ull + l_qname + 4ull * n_cigar + (uint64_t)(((int64_t)l_qseq + 1) / 2);
        if (at + (uint64_t)l_qseq > size) throw Undefined{"the qualities run past their record"};
        int64_t q = 0;
        for (int32_t i = 0; i < l_qseq; ++i) q += b[at + (uint64_t)i];
        return q;
    }
    // bam_aux_get(b, "RG"): the offset of the field's type byte, or 0.  __skip_tag upper-cases the type before it looks up the
    // size, so `d` has size 0 like every type it does not know; a B array's subtype is looked up as it is.
    uint64_t aux_rg() const
    {
        auto width = [](int t) { return t == 'C' || t == 'c' || t == 'A' ? 1 : t == 'S' || t == 's' ? 2 : t == 'I' || t == 'i' || t == 'f' || t == 'F' ? 4 : 0; };
        auto at = [&](uint64_t s) -> uint8_t {
            if (s >= size) throw Undefined{"an aux walk leaves its record"};
            return b[s];
        };
        uint64_t s = 36ull + l_qname + 4ull * n_cigar + (uint64_t)(((int64_t)l_qseq + 1) / 2) + (uint64_t)(int64_t)l_qseq;
        while (s < size) {
            const uint8_t t0 = at(s), t1 = at(s + 1);
            s += 2;
            if (t0 == 'R' && t1 == 'G') return s;
            const int t = toupper(at(s));
            ++s;
            if (t == 'Z' || t == 'H') {
                while (at(s)) ++s;
                ++s;
            } else if (t == 'B') {
                const int w = width(at(s));
                if (s + 5 > size) throw Undefined{"an aux walk leaves its record"};
                int32_t cnt;
                memcpy(&cnt, b + s + 1, 4);
                if (cnt < 0) throw Undefined{"an aux walk leaves its record"};
                s += 5 + (uint64_t)w * (uint64_t)cnt;
            } else {
                s += (uint64_t)width(t);
            }
        }
        return 0;
    }
};

// ---- the header's @RG lines ----

typedef std::vector<std::pair<std::string, std::string>> Tags;
struct HeaderLine {
    std::string type;
    Tags tags;
};

// sam_header_parse2: false where it gives up (its words go to `say`)
inline bool header_lines(const std::string &text, std::vector<HeaderLine> &lines, std::string &say)
{
    lines.clear();
    size_t at = 0;
    while (at < text.size()) {
        size_t to = at;
        while (to < text.size() && text[to] != '\n' && text[to] != '\r') ++to;
        const std::string line = text.substr(at, to - at);
        if (to < text.size()) {
            if (text[to] == '\n') ++to;
            else if (text.compare(to, 2, "\r\n") == 0) to += 2;
            else if (to == at) throw Undefined{"a lone CR in the header"};      // (nextline does not move: the reference loops for ever)
        }
        at = to;
        if (line.empty() || line[0] != '@') return say += "[sam_header_line_parse] expected '@', got [" + line + "]\n", false;
        size_t t = 1;
        while (t < line.size() && line[t] != '\t') ++t;
        if (t - 1 != 2) return say += "[sam_header_line_parse] expected '@XY', got [" + line + "]\nHint: The header tags must be tab-separated.\n", false;
        HeaderLine h;
        h.type = line.substr(1, 2);
        if (h.type != "HD" && h.type != "SQ" && h.type != "RG" && h.type != "PG" && h.type != "CO")
            throw Undefined{"a header line of unknown type"};      // (the reference reads its tag tables out of bounds)
        size_t p = 3;
        while (p < line.size() && line[p] == '\t') ++p;
        if (p - 3 != 1) return say += "[sam_header_line_parse] multiple tabs on line [" + line + "] (" + std::to_string(p - 3) + ")\n", false;
        if (h.type == "CO") {
            if (p < line.size()) h.tags.emplace_back("  ", line.substr(p));
        } else {
            while (p < line.size()) {
                size_t q = line.find('\t', p);
                if (q == std::string::npos) q = line.size();
                if (q - p < 3) throw Undefined{"a header tag shorter than XY:"};
                const std::string key = line.substr(p, 2);
                for (const auto &kv : h.tags)
                    if (kv.first == key) {
                        say += "The tag '" + key + "' present (at least) twice on line [" + line + "]\n";
                        break;
                    }
                h.tags.emplace_back(key, line.substr(p + 3, q - p - 3));
                size_t r = q;
                while (r < line.size() && line[r] == '\t') ++r;
                if (r < line.size() && r - q != 1)
                    return say += "[sam_header_line_parse] multiple tabs on line [" + line + "] (" + std::to_string(r - q) + ")\n", false;
                p = r;
            }
        }
        lines.push_back(h);
    }
    return !lines.empty();
}

// bam_get_library: the header is parsed on the first call -- and again on every call while parsing fails
class Libraries {
public:
    explicit Libraries(const std::string &text) : text_(text.c_str()) {}
    // the table ID -> LB; what the reference says while making it goes to `say`
    const std::map<std::string, std::string> &table(std::string &say)
    {
        if (!parsed_) parsed_ = header_lines(text_, lines_, say);
        if (!made_) {
            made_ = true;
            if (parsed_)
                for (const HeaderLine &h : lines_) {
                    if (h.type != "RG") continue;
                    const std::string *id = nullptr, *lb = nullptr;
                    for (const auto &kv : h.tags) {
                        if (!id && kv.first == "ID") id = &kv.second;
                        if (!lb && kv.first == "LB") lb = &kv.second;
                    }
                    if (!id || !lb) continue;
                    if (tbl_.count(*id)) say += "[sam_header_lookup_table] They key " + *id + " not unique.\n";
                    tbl_[*id] = *lb;
                }
        }
        return tbl_;
    }
    std::string of(const Rec &r)
    {
        std::string say;
        table(say);
        fputs(say.c_str(), stderr);
        const uint64_t rg = r.aux_rg();
        if (!rg) return "\t";
        const void *e = rg + 1 < r.size ? memchr(r.b + rg + 1, 0, r.size - rg - 1) : nullptr;
        if (!e) throw Undefined{"an RG value runs past its record"};
        const auto it = tbl_.find(std::string((const char *)r.b + rg + 1, (const char *)e));
        return it == tbl_.end() ? "\t" : it->second;
    }

private:
    std::string text_;
    std::vector<HeaderLine> lines_;
    std::map<std::string, std::string> tbl_;
    bool parsed_ = false, made_ = false;
};

// the table as the device route is given it; false where the header is not parsed in silence (the host route says what the
// reference says, at every head again)
inline bool id_table(const std::string &text, std::map<std::string, std::string> &tbl)
{
    std::string say;
    try {
        Libraries l(text);
        tbl = l.table(say);
    } catch (const Undefined &) {
        return false;
    }
    return say.empty();
}

// ---- khash's order over strings ----

inline uint32_t x31(const std::string &s)
{
    uint32_t h = s.empty() ? 0u : (uint32_t)(int32_t)(signed char)s[0];
    for (size_t k = 1; k < s.size(); ++k) h = (h << 5) - h + (uint32_t)(int32_t)(signed char)s[k];
    return h;
}

// the bucket order of a khash 0.2.5 string table that only grows (kh_put, kh_resize)
class KhStrings {
public:
    void put(const std::string &key)
    {
        for (size_t i = 0; i < keys_.size(); ++i)
            if (used_[i] && keys_[i] == key) return;
        if (size_ >= upper_) resize(nb_ > (size_ << 1) ? nb_ - 1 : nb_ + 1);
        const uint32_t k = x31(key), inc = 1 + k % (nb_ - 1);
        uint32_t i = k % nb_;
        while (used_[i]) i = i + inc >= nb_ ? i + inc - nb_ : i + inc;
        keys_[i] = key, used_[i] = true;
        ++size_;
    }
    std::vector<std::string> order() const
    {
        std::vector<std::string> out;
        for (size_t i = 0; i < keys_.size(); ++i)
            if (used_[i]) out.push_back(keys_[i]);
        return out;
    }

private:
    void resize(uint32_t want)
    {
        static const uint32_t primes[32] = {0u,        3u,        11u,       23u,        53u,        97u,        193u,       389u,       769u,        1543u,      3079u,
                                            6151u,     12289u,    24593u,    49157u,     98317u,     196613u,    393241u,    786433u,    1572869u,    3145739u,   6291469u,
                                            12582917u, 25165843u, 50331653u, 100663319u, 201326611u, 402653189u, 805306457u, 1610612741u, 3221225473u, 4294967291u};
        int t = 31;
        while (primes[t] > want) --t;
        const uint32_t nb = primes[t + 1];
        if (size_ >= (uint32_t)(nb * 0.77 + 0.5)) return;
        std::vector<std::string> old(keys_);
        old.resize(nb > nb_ ? nb : nb_);
        std::vector<char> moved(old.size(), 1), fresh(nb, 0);
        for (uint32_t j = 0; j < nb_; ++j) moved[j] = !used_[j];
        for (uint32_t j = 0; j < nb_; ++j) {
            if (moved[j]) continue;
            std::string key = old[j];
            moved[j] = 1;
            for (;;) {
                const uint32_t k = x31(key), inc = 1 + k % (nb - 1);
                uint32_t i = k % nb;
                while (fresh[i]) i = i + inc >= nb ? i + inc - nb : i + inc;
                fresh[i] = 1;
                if (i < nb_ && !moved[i]) {
                    std::swap(old[i], key);
                    moved[i] = 1;
                } else {
                    old[i] = key;
                    break;
                }
            }
        }
        keys_.assign(old.begin(), old.begin() + nb);
        used_.assign(fresh.begin(), fresh.end());
        nb_ = nb, upper_ = (uint32_t)(nb * 0.77 + 0.5);
    }
    uint32_t nb_ = 0, size_ = 0, upper_ = 0;
    std::vector<std::string> keys_;
    std::vector<char> used_;
};

struct LibCount {
    uint64_t removed = 0, checked = 0;
};

// the lines behind the last record, one per library in the table's order; first_seen: the libraries as their first record came
inline void library_lines(const char *core, const std::map<std::string, LibCount> &counts, const std::vector<std::string> &first_seen)
{
    KhStrings kh;
    for (const std::string &l : first_seen) kh.put(l);
    for (const std::string &l : kh.order()) {
        const LibCount &q = counts.at(l);
        fprintf(stderr, "[%s] %lld / %lld = %.4lf in library '%s'\n", core, (long long)q.removed, (long long)q.checked, (double)q.removed / (double)q.checked, l.c_str());
    }
}

// ---- the two cores: the ordinals of the records they write, in output order ----

inline std::vector<uint32_t> core_pairs(const std::vector<Rec> &recs, const bamsort::Header &hdr)
{
    struct Slot {
        uint32_t rec;
        bool written;
    };
    std::vector<uint32_t> out;
    std::vector<std::shared_ptr<Slot>> stack;
    std::unordered_set<std::string> del_set;
    std::map<std::string, std::unordered_map<uint64_t, std::shared_ptr<Slot>>> best;
    std::map<std::string, LibCount> counts;
    std::vector<std::string> seen;
    Libraries libs(hdr.text);
    int32_t last_tid = -1, last_pos = -1;
    auto dump = [&]() {
        for (auto &s : stack) out.push_back(s->rec), s->written = true;
        stack.clear();
    };
    for (size_t i = 0; i < recs.size(); ++i) {
        const Rec &r = recs[i];
        if (r.tid != last_tid || r.pos != last_pos) {
            dump();
            for (auto &h : best)
                if (h.second.size() >= 0x40000) h.second.clear();
            if (r.tid != last_tid) {
                for (auto &h : best) h.second.clear();
                if (!del_set.empty()) {
                    fprintf(stderr, "[bam_rmdup_core] %llu unmatched pairs\n", (unsigned long long)del_set.size());
                    del_set.clear();
                }
                if (r.tid == -1) {
                    for (size_t k = i; k < recs.size(); ++k) out.push_back((uint32_t)k);
                    break;
                }
                last_tid = r.tid;
                if (r.tid < 0 || (size_t)r.tid >= hdr.name.size()) throw Undefined{"a refID the header does not have"};
                fprintf(stderr, "[bam_rmdup_core] processing reference %s...\n", hdr.name[(size_t)r.tid].c_str());
            }
        }
        if (!(r.flag & 1) || (r.flag & 12) || (r.mtid >= 0 && r.tid != r.mtid)) {
            out.push_back((uint32_t)i);
        } else if (r.isize > 0) {
            const std::string lib = libs.of(r);
            if (!counts.count(lib)) counts[lib] = LibCount(), best[lib], seen.push_back(lib);
            ++counts[lib].checked;
            const uint64_t key = (uint64_t)(uint32_t)r.pos << 32 | (uint32_t)r.isize;
            auto &h = best[lib];
            const auto it = h.find(key);
            if (it != h.end()) {
                Slot &s = *it->second;
                if (s.written) throw Undefined{"a stale best_hash key is hit: the reference reads a record it has freed (the input is not sorted by coordinate)"};
                ++counts[lib].removed;
                std::string name;
                if (recs[s.rec].sum_qual() < r.sum_qual()) name = recs[s.rec].name(), s.rec = (uint32_t)i;
                else name = r.name();
                if (!del_set.insert(name).second)
                    fprintf(stderr, "[bam_rmdup_core] inconsistent BAM file for pair '%s'. Continue anyway.\n", r.name().c_str());
            } else {
                auto s = std::make_shared<Slot>(Slot{(uint32_t)i, false});
                h.emplace(key, s);
                stack.push_back(s);
            }
        } else if (!del_set.erase(r.name())) {
            out.push_back((uint32_t)i);
        }
        last_pos = r.pos;
    }
    dump();
    library_lines("bam_rmdup_core", counts, seen);
    return out;
}

// The queue is a klist: a node that leaves goes to a pool and is the next one taken, and the tables may still point at it.
inline std::vector<uint32_t> core_single(const std::vector<Rec> &recs, const bamsort::Header &hdr, bool force_se)
{
    struct Node {
        int32_t endpos = 0;
        uint32_t score = 0, rec = 0;
        bool discarded = false;
    };
    constexpr int32_t kMaxPos = 0x7fffffff;
    std::vector<uint32_t> out;
    std::vector<std::unique_ptr<Node>> owned;
    std::vector<Node *> queue, pool;
    size_t head = 0;
    struct Tables {
        std::unordered_map<uint32_t, Node *> left, right;
    };
    std::map<std::string, Tables> tables;
    std::map<std::string, LibCount> counts;
    std::vector<std::string> seen;
    Libraries libs(hdr.text);
    int32_t last_tid = -2;
    auto push = [&](uint32_t i, int32_t endpos, int64_t score) {
        Node *n;
        if (pool.empty()) owned.emplace_back(new Node), n = owned.back().get();
        else n = pool.back(), pool.pop_back();
        n->endpos = endpos, n->score = (uint32_t)score & 0x7fffffffu, n->discarded = false, n->rec = i;
        queue.push_back(n);
        return n;
    };
    auto dump = [&](int32_t pos) {
        if (queue.size() - head <= 0x100000 && pos != kMaxPos) return;
        while (head < queue.size()) {
            Node *n = queue[head];
            if (!n->discarded) {
                if ((recs[n->rec].flag & 16) && n->endpos > pos) break;
                out.push_back(n->rec);
            }
            ++head;
            pool.push_back(n);
        }
        if (head > (1u << 16)) queue.erase(queue.begin(), queue.begin() + (ptrdiff_t)head), head = 0;
        for (auto &t : tables)
            for (auto *h : {&t.second.left, &t.second.right})
                for (auto it = h->begin(); it != h->end();) it = it->second->endpos <= pos ? h->erase(it) : std::next(it);
    };
    for (size_t i = 0; i < recs.size(); ++i) {
        const Rec &r = recs[i];
        if (36ull + r.l_qname + 4ull * r.n_cigar > r.size) throw Undefined{"a CIGAR runs past its record"};
        const int32_t endpos = (int32_t)bai::calend(r.pos, r.b + 36 + r.l_qname, r.n_cigar);
        const int64_t score = r.sum_qual();
        if (last_tid != r.tid) {
            if (last_tid >= 0) dump(kMaxPos);
            last_tid = r.tid;
        } else {
            dump(r.pos);
        }
        if ((r.flag & 4) || ((r.flag & 1) && !force_se)) {
            push((uint32_t)i, endpos, score);
            continue;
        }
        const std::string lib = libs.of(r);
        if (!counts.count(lib)) counts[lib] = LibCount(), tables[lib], seen.push_back(lib);
        ++counts[lib].checked;
        const bool rev = (r.flag & 16) != 0;
        auto &h = rev ? tables[lib].right : tables[lib].left;
        const uint32_t key = rev ? (uint32_t)endpos : (uint32_t)r.pos;
        const auto it = h.find(key);
        if (it == h.end()) {
            h[key] = push((uint32_t)i, endpos, score);
            continue;
        }
        ++counts[lib].removed;
        Node *n = it->second;
        if ((int64_t)n->score < score) {
            if (rev) n->discarded = true, it->second = push((uint32_t)i, endpos, score);
            else n->score = (uint32_t)score & 0x7fffffffu, n->endpos = endpos, n->rec = (uint32_t)i;
        }
    }
    dump(kMaxPos);
    library_lines("bam_rmdupse_core", counts, seen);
    return out;
}

// `samtools rmdup` behind its argument check.  Returns the status (0, 1 as the reference; 2 where the reference's behaviour is
// undefined or it crashes: no output is left).
inline int rmdup_on_host(const Options &o)
{
    FILE *f = fopen(strcmp(o.in, "-") ? o.in : "/dev/stdin", "rb");
    if (!f) {
        fprintf(stderr, "[hpn] bam_rmdup: %s: %s (the reference ends with a segmentation fault here)\n", o.in, strerror(errno));
        return 2;
    }
    const bool eof_marker = bai::has_eof_marker(f);
    bai::BgzfSeq z(f);
    bamsort::Header hdr;
    const int hr = bamsort::read_header(z, hdr);
    if (hr != 0) {
        fclose(f);
        fprintf(stderr, "[hpn] bam_rmdup: %s: outside the tool's domain\n", hr == -1 ? "the input is no BAM file" : "the header ends early");
        return 2;
    }
    if (!eof_marker) fputs("[bam_header_read] EOF marker is absent. The input is probably truncated.\n", stderr);
    // every record, as bam_read1 takes them (the loop of either core ends without a word where one is cut short)
    std::vector<uint8_t> buf;
    std::vector<std::pair<uint64_t, uint32_t>> where;
    for (;;) {
        int32_t block_len;
        if (z.read(&block_len, 4) != 4) break;
        uint32_t x[8];
        if (z.read(x, 32) != 32) break;
        const int64_t want = (int64_t)block_len - 32;
        if (want < 0) break;
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
            break;
        }
        where.emplace_back(at, (uint32_t)block_len + 4u);
    }
    fclose(f);
    std::vector<Rec> recs;
    recs.reserve(where.size());
    for (const auto &w : where) recs.emplace_back(&buf[w.first], w.second);
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), -1, head_blocks)) {
        fputs("[hpn] bam_rmdup: deflating the header failed\n", stderr);
        return 2;
    }
    const bool to_stdout = strcmp(o.out, "-") == 0;
    BgzfWriter w(-1);
    if (!w.begin(to_stdout ? "/dev/stdout" : o.out, head_blocks)) {      // (the reference opens its output before it reads a record)
        fputs("[bam_rmdup] fail to read/write input files\n", stderr);
        return 1;
    }
    std::vector<uint32_t> order;
    try {
        order = o.se ? core_single(recs, hdr, o.force_se) : core_pairs(recs, hdr);
    } catch (const Undefined &u) {
        fprintf(stderr, "[hpn] bam_rmdup: %s: the reference's behaviour is undefined here, nothing is written\n", u.what.c_str());
        w.abandon();
        if (!to_stdout) unlink(o.out);
        return 2;
    }
    auto emit = [&](const uint8_t *p, uint32_t n) { w.add(p, n, 0, false); };
    BgzfCutter<decltype(emit)> cut(emit);
    for (uint32_t k : order) cut.record(recs[k].b, recs[k].size);
    cut.close();
    if (!w.finish()) {
        fprintf(stderr, "[hpn] bam_rmdup: writing %s failed\n", o.out);
        return 2;
    }
    return 0;
}

}  // namespace rmdup
}  // namespace hpn
