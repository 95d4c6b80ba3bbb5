// kseq_read.hpp -- klib's kseq_read as map_kseq.cpp and kbtree_kseq.c call it, over a stream in memory, and the two programs'
// answer through a std::map: where text that the device does not frame goes (wrapped FASTQ, mixed '>' and '@' records, a
// truncated tail, a quality of another length, sequences beyond 65,535 bytes).  Header-only, no HIP.
//
// The two programs hand kseq_read a NEW, zeroed record every time.  What follows from that is restated here, not only the
// parser's own rules:
//   - the record has forgotten that the sequence loop of the call before consumed the next header's first byte, so every call
//     looks for the next '>' or '@' at ANY byte: behind a FASTA record the next header line is passed over;
//   - a comment that was never read is a NULL pointer, and so is the quality of a FASTA record: "%s" prints "(null)";
//   - the name runs to the first isspace byte; unless that byte is '\n' the rest of the line is the comment, and a comment that
//     the stream's end leaves without a single byte to read stays NULL;
//   - sequence lines are appended up to a line that starts with '>', '+' or '@' (that byte is consumed), empty lines skipped;
//   - a line read to its end loses a trailing '\r' when what has accumulated is longer than 1 byte -- but a line whose first
//     byte is the stream's last byte is not "read to its end": nothing is dropped there;
//   - behind a '+' line (skipped; a stream that ends in it: -2) quality lines are appended, at least one, until they reach the
//     sequence's length; another length: -2.  Both programs stop at the first negative return.
#pragma once
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>

namespace hpn {

struct KseqRecord {
    std::string name, comment, seq, qual;
    bool has_comment = false, has_qual = false;
};

class KseqReader {
public:
    KseqReader(const char *data, size_t n) : d_(data), n_(n) {}

    // the sequence's length, -1 at the stream's end, -2 for a truncated or ragged quality
    long read(KseqRecord &r)
    {
        r = KseqRecord();
        while (pos_ < n_ && d_[pos_] != '>' && d_[pos_] != '@') ++pos_;
        if (pos_ == n_) return -1;
        ++pos_;
        if (pos_ == n_) return -1;   // a header's first byte ends the stream
        size_t i = pos_;
        while (i < n_ && !space(d_[i])) ++i;
        r.name.assign(d_ + pos_, i - pos_);
        const int stop = i < n_ ? (unsigned char)d_[i] : 0;
        pos_ = i < n_ ? i + 1 : n_;
        if (stop != '\n' && pos_ < n_) {
            r.has_comment = true;
            line_to(r.comment);
        }
        while (pos_ < n_) {
            const char c = d_[pos_++];
            if (c == '>' || c == '+' || c == '@') {
                if (c != '+') return (long)r.seq.size();
                return quality(r);
            }
            if (c == '\n') continue;
            r.seq.push_back(c);
            if (pos_ < n_) line_to(r.seq);
        }
        return (long)r.seq.size();
    }

private:
    static bool space(char c) { return c == ' ' || (c >= 9 && c <= 13); }

    // appends the rest of the line (there is at least one byte to read), passes its '\n', applies the '\r' rule
    void line_to(std::string &s)
    {
        const char *e = (const char *)memchr(d_ + pos_, '\n', n_ - pos_);
        const size_t stop = e ? (size_t)(e - d_) : n_;
        s.append(d_ + pos_, stop - pos_);
        pos_ = e ? stop + 1 : n_;
        if (s.size() > 1 && s.back() == '\r') s.pop_back();
    }

    long quality(KseqRecord &r)
    {
        const char *e = (const char *)memchr(d_ + pos_, '\n', n_ - pos_);
        if (!e) {
            pos_ = n_;
            return -2;
        }
        pos_ = (size_t)(e - d_) + 1;
        r.has_qual = true;
        do {
            if (pos_ == n_) break;
            line_to(r.qual);
        } while (r.qual.size() < r.seq.size());
        return r.qual.size() == r.seq.size() ? (long)r.seq.size() : -2;
    }

    const char *d_;
    size_t n_, pos_ = 0;
};

struct KseqAnswer {
    uint64_t n_records = 0, n_distinct = 0;
    bool one_length = true;
    size_t first_len = 0, other_len = 0;   // the first record's length; with !one_length the first one that differs
    std::string out;                       // "name comment\nseq\n+\nqual\n" per distinct sequence, in the sequences' order
};

// map_kseq.cpp's answer for a stream without NUL bytes (the caller refuses those: "%s" would cut the line there)
inline KseqAnswer kseq_map(const char *data, size_t n)
{
    KseqAnswer a;
    std::map<std::string, KseqRecord> first;
    KseqReader in(data, n);
    KseqRecord r;
    while (in.read(r) >= 0) {
        if (!a.n_records) a.first_len = r.seq.size();
        else if (a.one_length && r.seq.size() != a.first_len) a.one_length = false, a.other_len = r.seq.size();
        ++a.n_records;
        if (!first.count(r.seq)) first.emplace(r.seq, std::move(r));
    }
    a.n_distinct = first.size();
    for (const auto &kv : first) {
        const KseqRecord &x = kv.second;
        a.out.append(x.name).push_back(' ');
        a.out.append(x.has_comment ? x.comment : std::string("(null)")).push_back('\n');
        a.out.append(x.seq).append("\n+\n");
        a.out.append(x.has_qual ? x.qual : std::string("(null)")).push_back('\n');
    }
    return a;
}

}  // namespace hpn
