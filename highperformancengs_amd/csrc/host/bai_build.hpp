// bai_build.hpp -- samtools-0.1.19's `index` on the host: the sequential indexer (the route of HPN_BAM_GPU=0 and the fallback of
// bin/bam_index), the order in which a target's bins are written, the .bai writer and the reference's messages.
// (docs/kernels/bam_bai.md states the rules; tests/bai_ref.py is the same in Python, tests/golden/bai/ the recorded runs.)
//
// The file is read the way bgzf_read reads it, because the index is made of what bam_tell says between two records:
//   - a record's start offset is the end offset of the record before it, the first one is the offset behind the header;
//   - the end offset of a record whose last byte lies in block k is addr[k] << 16 | bytes into the block, and addr[k + 1] << 16
//     where the record ends with the block (the reader moves on to the next block's address at once);
//   - a block of no bytes ends the stream for the reader, wherever it lies: the file's EOF marker, or an empty block in mid-file.
// Nothing here needs a GPU: tests/bai_host_main.cpp builds this header alone.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace hpn {
namespace bai {

constexpr uint32_t kMetaBin = 37450;      // one past the last bin of the scheme: (offsets, counts) of the target

struct Chunk {
    uint64_t beg, end;
};

// Where the keys of samtools' bin table (khash, integer keys, nothing ever deleted) lie: bucket counts from a list of primes,
// slot = key mod n, step = 1 + key mod (n - 1), grown when 0.77 n slots are taken.  The index lists a target's bins slot by
// slot, so the order of the file is the order of the slots after the last insertion.
class KhOrder {
public:
    bool put(uint32_t key)        // true: the key is new
    {
        if (size_ >= upper_) grow();
        uint32_t i = key % n_;
        if (used_[i]) {
            const uint32_t inc = 1 + key % (n_ - 1);
            while (used_[i] && keys_[i] != key) i = i + inc >= n_ ? i + inc - n_ : i + inc;
        }
        if (used_[i]) return false;
        keys_[i] = key, used_[i] = 1, ++size_;
        return true;
    }
    void order(std::vector<uint32_t> &out) const
    {
        out.clear();
        for (uint32_t i = 0; i < n_; ++i)
            if (used_[i]) out.push_back(keys_[i]);
    }

private:
    void grow()
    {
        static const uint32_t primes[] = {0u,        3u,        11u,       23u,       53u,        97u,        193u,       389u,
                                          769u,      1543u,     3079u,     6151u,     12289u,     24593u,     49157u,     98317u,
                                          196613u,   393241u,   786433u,   1572869u,  3145739u,   6291469u,   12582917u,  25165843u,
                                          50331653u, 100663319u, 201326611u, 402653189u, 805306457u, 1610612741u, 3221225473u, 4294967291u};
        int t = 31;
        while (primes[t] > n_ + 1) --t;
        const uint32_t nn = primes[t + 1];
        if (size_ >= (uint32_t)(nn * 0.77 + 0.5)) return;
        keys_.resize(nn, 0);
        std::vector<uint8_t> old(used_), now(nn, 0);      // old: holds a key that has not moved yet
        for (uint32_t j = 0; j < n_; ++j) {
            if (!old[j]) continue;
            uint32_t key = keys_[j];
            old[j] = 0;
            for (;;) {                                    // a key that lands on an unmoved one takes its slot and sends it on
                uint32_t i = key % nn;
                const uint32_t inc = 1 + key % (nn - 1);
                while (now[i]) i = i + inc >= nn ? i + inc - nn : i + inc;
                now[i] = 1;
                if (i < n_ && old[i]) {
                    std::swap(keys_[i], key);
                    old[i] = 0;
                } else {
                    keys_[i] = key;
                    break;
                }
            }
        }
        used_.swap(now);
        n_ = nn, upper_ = (uint32_t)(nn * 0.77 + 0.5);
    }
    uint32_t n_ = 0, size_ = 0, upper_ = 0;
    std::vector<uint32_t> keys_;
    std::vector<uint8_t> used_;
};

// One target of the index: its bins in the order in which their first chunk closed (the metadata bin last), every bin's chunks
// in file order, the linear index (0: an empty window) and its length.
struct TargetIndex {
    std::vector<std::pair<uint32_t, std::vector<Chunk>>> bins;
    std::vector<uint64_t> lin;
    int32_t n_lin = 0;
};

struct Index {
    std::vector<TargetIndex> t;
    uint64_t n_no_coor = 0;
};

// chunk l joins the one before it where that one ends in the BGZF block this one starts in (the metadata bin is left alone)
inline void merge_chunks(std::vector<Chunk> &v)
{
    size_t m = 0;
    for (size_t l = 1; l < v.size(); ++l) {
        if (v[m].end >> 16 == v[l].beg >> 16) v[m].end = v[l].end;
        else v[++m] = v[l];
    }
    if (!v.empty()) v.resize(m + 1);
}

// empty windows take the offset of the window before them; window 0 stays empty if it is
inline void fill_windows(uint64_t *lin, int64_t n)
{
    for (int64_t j = 1; j < n; ++j)
        if (lin[j] == 0) lin[j] = lin[j - 1];
}

// The file: every list is final (merged, filled).  false: a write failed.
inline bool write_index(const Index &ix, FILE *f)
{
    std::vector<uint8_t> out;
    auto put = [&](const void *p, size_t n) { out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + n); };
    const int32_t n_ref = (int32_t)ix.t.size();
    put("BAI\1", 4), put(&n_ref, 4);
    std::vector<uint32_t> order;
    for (const TargetIndex &t : ix.t) {
        KhOrder table;
        std::unordered_map<uint32_t, size_t> at;
        for (size_t k = 0; k < t.bins.size(); ++k) table.put(t.bins[k].first), at[t.bins[k].first] = k;
        // The table grows at the START of an insertion that finds it full, also one of a key it already holds, and a target's
        // last insertion is always such a one (the metadata bin's second entry): a table left exactly full grows once more.
        if (!t.bins.empty()) table.put(t.bins.back().first);
        table.order(order);
        const int32_t n_bin = (int32_t)order.size();
        put(&n_bin, 4);
        for (uint32_t b : order) {
            const std::vector<Chunk> &ch = t.bins[at[b]].second;
            const int32_t n_chunk = (int32_t)ch.size();
            put(&b, 4), put(&n_chunk, 4);
            if (n_chunk) put(ch.data(), (size_t)n_chunk * sizeof(Chunk));
        }
        put(&t.n_lin, 4);
        if (t.n_lin > 0) put(t.lin.data(), (size_t)t.n_lin * 8);
        if (out.size() > ((size_t)8 << 20)) {
            if (fwrite(out.data(), 1, out.size(), f) != out.size()) return false;
            out.clear();
        }
    }
    put(&ix.n_no_coor, 8);
    return fwrite(out.data(), 1, out.size(), f) == out.size() && fflush(f) == 0;
}

// The inflated stream of a BGZF file as samtools' reader presents it, with the virtual offset it reports at any moment.
// Three properties of that reader make the index what it is, and this class keeps exactly them:
//   - a block is fetched only when a byte of it is wanted;
//   - the moment the last byte of a block has been handed out, the position is the NEXT block's file offset with 0 bytes in;
//   - a block of no bytes (and the end of the file) hands out nothing: the request that met it comes back short.
// Blocks must carry the plain 18-byte header (XLEN 6, one BC subfield of 2 bytes); their CRC-32 and ISIZE are not looked at.
class BgzfSeq {
public:
    explicit BgzfSeq(FILE *f) : file_(f) {}

    // up to n bytes into dst: how many there were, or -1 when a block is damaged or cut off
    int64_t read(void *dst, int64_t n)
    {
        if (n <= 0) return 0;
        uint8_t *out = (uint8_t *)dst;
        int64_t done = 0;
        for (;;) {
            if (used_ == size_ && (!fetch() || size_ == 0)) {
                if (broken_) return -1;
                break;                                   // nothing more: the file's end or a block of no bytes
            }
            const int64_t piece = std::min<int64_t>(n - done, (int64_t)(size_ - used_));
            memcpy(out + done, bytes_ + used_, (size_t)piece);
            used_ += (uint32_t)piece, done += piece;
            if (done == n) break;
        }
        if (used_ == size_) block_at_ = file_at_, used_ = size_ = 0;      // used up: the reader already stands at the next block
        return done;
    }
    uint64_t tell() const { return block_at_ << 16 | used_; }

private:
    static bool plain_header(const uint8_t *h)
    {
        const bool gzip_extra = h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4);
        return gzip_extra && (h[10] | h[11] << 8) == 6 && h[12] == 'B' && h[13] == 'C' && (h[14] | h[15] << 8) == 2;
    }
    // the next block of the file into bytes_ (size_ = 0 at the end of the file); false and broken_ when it cannot be had
    bool fetch()
    {
        const uint64_t here = file_at_;
        uint8_t head[18];
        const size_t got = fread(head, 1, sizeof head, file_);
        file_at_ += got;
        used_ = size_ = 0;
        if (got == 0) return true;
        if (got != sizeof head || !plain_header(head)) return broken_ = true, false;
        const size_t whole_block = (size_t)(head[16] | head[17] << 8) + 1;               // BSIZE + 1
        if (whole_block < sizeof head) return broken_ = true, false;
        const size_t rest = whole_block - sizeof head;
        const size_t body = fread(packed_, 1, rest, file_);
        file_at_ += body;
        if (body != rest) return broken_ = true, false;
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return broken_ = true, false;
        zs.next_in = packed_, zs.avail_in = (uInt)rest;
        zs.next_out = bytes_, zs.avail_out = sizeof bytes_;
        const bool whole = inflate(&zs, Z_FINISH) == Z_STREAM_END;
        const uint32_t made = (uint32_t)zs.total_out;
        inflateEnd(&zs);
        if (!whole) return broken_ = true, false;
        block_at_ = here, size_ = made;
        return true;
    }
    FILE *file_;
    uint64_t file_at_ = 0, block_at_ = 0;      // where the file is read next; where the block in bytes_ starts
    uint32_t size_ = 0, used_ = 0;
    bool broken_ = false;
    uint8_t packed_[65536], bytes_[65536];
};

// Where a record ends on the reference, as the 32-bit unsigned number the linear index takes it for: pos plus the lengths of the
// operations that consume the reference (M D N = X).  An operation `B` of length b steps back over the last b bases of the READ:
// the end moves left by the reference bases those cover (walked from the `B` towards the CIGAR's start; an operation that
// holds the b-th base counts only its share), and to pos itself when the CIGAR in front of the `B` is shorter than b bases.
// A `B` as the very last operation ends the walk.
inline uint32_t calend(int32_t pos, const uint8_t *cigar, uint32_t n_cigar)
{
    constexpr uint32_t kReadBit = 1, kRefBit = 2, kBack = 9;
    auto op_of = [&](uint32_t k) { uint32_t v; memcpy(&v, cigar + 4 * (size_t)k, 4); return v; };
    auto consumes = [](uint32_t word) { return 0x3C1A7u >> ((word & 15u) << 1) & 3u; };
    uint32_t end = (uint32_t)pos;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t word = op_of(k);
        if ((word & 15u) != kBack) {
            if (consumes(word) & kRefBit) end += word >> 4;
            continue;
        }
        if (k + 1 == n_cigar) break;
        const int64_t want = word >> 4;
        int64_t read_bases = 0, ref_bases = 0;
        bool found = false;
        for (uint32_t j = k; j-- > 0;) {
            const uint32_t w = op_of(j), c = consumes(w);
            const int64_t len = w >> 4;
            if ((c & kReadBit) && read_bases + len >= want) {
                if (c & kRefBit) ref_bases += want - read_bases;
                found = true;
                break;
            }
            if (c & kReadBit) read_bases += len;
            if (c & kRefBit) ref_bases += len;
        }
        end = found ? end - (uint32_t)ref_bases : (uint32_t)pos;
    }
    return end;
}

struct Record {
    int32_t tid = 0, pos = 0;
    uint32_t bin = 0, flag = 0, l_name = 0, n_cigar = 0;
    std::vector<uint8_t> data;      // behind the 32 fixed bytes
};

// bam_read1: 4 + block_size, or its negative codes (-1 the stream ends, -2 / -3 / -4 it ends inside a record)
inline int64_t read1(BgzfSeq &z, Record &r)
{
    int32_t block_len;
    const int64_t got = z.read(&block_len, 4);
    if (got != 4) return got == 0 ? -1 : -2;
    uint32_t x[8];
    if (z.read(x, 32) != 32) return -3;
    r.tid = (int32_t)x[0], r.pos = (int32_t)x[1];
    r.bin = x[2] >> 16, r.l_name = x[2] & 0xffu, r.flag = x[3] >> 16, r.n_cigar = x[3] & 0xffffu;
    const int64_t want = (int64_t)block_len - 32;
    r.data.clear();
    if (want < 0) return -4;                       // (a read of no bytes is short of a negative count)
    for (int64_t have = 0; have < want;) {         // in pieces: a damaged size word does not allocate 2 GB
        const int64_t k = want - have < (1 << 20) ? want - have : (1 << 20);
        r.data.resize((size_t)(have + k));
        const int64_t g = z.read(r.data.data() + have, k);
        if (g != k) return -4;
        have += k;
    }
    return 4 + (int64_t)block_len;
}

enum { kDone = 0, kFailed = 1, kRefused = 2 };

// The index of one file, grown record by record.  The caller hands over every record with the virtual offset at which it
// starts (`at`) and the one behind it (`after`); what is kept between two records is the open run -- the records since the
// last change of (refID, stored bin), which become one chunk when the next run starts --, the open target's counts and the
// offset at which it began, and the record before (for the order checks).
class Indexer {
public:
    Indexer(Index &ix, int32_t n_ref, uint64_t first_offset) : ix_(ix), slot_((size_t)n_ref), target_from_(first_offset)
    {
        ix_.t.assign((size_t)n_ref, TargetIndex());
        ix_.n_no_coor = 0;
    }

    enum Step { kGoOn, kUnplacedFrom, kNotSorted, kStuck, kUndefined };
    std::string said;        // the reference's message (kNotSorted, kStuck), or why the reference's behaviour is undefined

    // one record of the file's placed part; kUnplacedFrom: this is the first record without a refID, the placed part is over
    Step add(const Record &r, uint64_t at, uint64_t after)
    {
        const int32_t n_ref = (int32_t)ix_.t.size();
        if (r.tid < -1 || r.tid >= n_ref) return undefined("a record's refID is outside the header's targets");
        if (r.tid < 0) ++ix_.n_no_coor;
        // a refID that goes up, or from a target to none, starts a new target; anything else must keep the order
        const bool new_target = seen_tid_ < r.tid || (seen_tid_ >= 0 && r.tid < 0);
        if (new_target) {
            seen_tid_ = r.tid;
        } else if ((uint32_t)seen_tid_ > (uint32_t)r.tid) {
            return not_sorted(r, "%d-th chr > %d-th chr", (long long)seen_tid_ + 1, (long long)r.tid + 1, 0);
        } else if (r.tid >= 0 && seen_pos_ > r.pos) {
            return not_sorted(r, "%u > %u in %d-th chr", (long long)(uint32_t)seen_pos_, (long long)(uint32_t)r.pos, r.tid + 1);
        }
        const bool mapped = r.tid >= 0 && !(r.flag & 4u);
        if (mapped) {
            if (r.pos < 0) return undefined("a mapped record with a negative position");
            if ((size_t)r.l_name + 4 * (size_t)r.n_cigar > r.data.size()) return undefined("a record's name and CIGAR do not fit its size");
            reach_windows(ix_.t[(size_t)r.tid], r, at);
        }
        if (!run_open_ || new_target || r.bin != run_bin_) {
            if (run_open_) {
                chunk(run_tid_, run_bin_, run_from_, at);
                if (new_target) close_target(at);
            }
            run_open_ = true, run_tid_ = r.tid, run_bin_ = r.bin, run_from_ = at;
            if (r.tid < 0) return kUnplacedFrom;
        }
        if (after <= at) {
            char line[160];
            snprintf(line, sizeof line, "[bam_index_core] bug in BGZF/RAZF: %llx < %llx\n", (unsigned long long)after, (unsigned long long)at);
            said = line;
            return kStuck;
        }
        ++(r.flag & 4u ? unmapped_ : mapped_);
        seen_pos_ = r.pos;
        return kGoOn;
    }

    // the stream of placed records is over at offset `end`: the open run and its target are closed, the lists made final
    void finish(uint64_t end)
    {
        if (run_open_ && run_tid_ >= 0) {
            chunk(run_tid_, run_bin_, run_from_, end);
            close_target(end);
        }
        for (TargetIndex &t : ix_.t) {
            for (auto &b : t.bins)
                if (b.first != kMetaBin) merge_chunks(b.second);
            fill_windows(t.lin.data(), t.n_lin);
        }
    }

private:
    Step undefined(const char *why)
    {
        said = std::string("bam_index: ") + why + ": outside the tool's domain\n";
        return kUndefined;
    }
    Step not_sorted(const Record &r, const char *what, long long a, long long b, int c)
    {
        const uint8_t *nul = (const uint8_t *)memchr(r.data.data(), 0, r.data.size());
        if (!nul) return undefined("a read name without its end");
        char tail[96];
        snprintf(tail, sizeof tail, what, (unsigned)a, (unsigned)b, c);
        said = "[bam_index_core] the alignment is not sorted (" + std::string((const char *)r.data.data(), (size_t)(nul - r.data.data())) + "): " + tail + "\n";
        return kNotSorted;
    }
    // the 16 kb windows from the record's first base to its last take its offset where they have none yet; the target's
    // window count becomes this record's last window + 1, whatever it was
    static void reach_windows(TargetIndex &t, const Record &r, uint64_t at)
    {
        const int32_t first = r.pos >> 14, last = (int32_t)((calend(r.pos, r.data.data() + r.l_name, r.n_cigar) - 1u) >> 14);
        if ((int64_t)t.lin.size() <= (int64_t)last) t.lin.resize((size_t)last + 1, 0);
        for (int32_t w = first; w <= last; ++w)
            if (!t.lin[(size_t)w]) t.lin[(size_t)w] = at;
        t.n_lin = last + 1;
    }
    void chunk(int32_t tid, uint32_t bin, uint64_t from, uint64_t to)
    {
        TargetIndex &t = ix_.t[(size_t)tid];
        auto found = slot_[(size_t)tid].find(bin);
        if (found == slot_[(size_t)tid].end()) {
            found = slot_[(size_t)tid].emplace(bin, t.bins.size()).first;
            t.bins.emplace_back(bin, std::vector<Chunk>());
        }
        t.bins[found->second].second.push_back(Chunk{from, to});
    }
    void close_target(uint64_t at)
    {
        chunk(run_tid_, kMetaBin, target_from_, at);
        chunk(run_tid_, kMetaBin, mapped_, unmapped_);
        mapped_ = unmapped_ = 0;
        target_from_ = at;
    }
    Index &ix_;
    std::vector<std::unordered_map<uint32_t, size_t>> slot_;      // per target: where a bin's list lies in TargetIndex::bins
    bool run_open_ = false;
    int32_t run_tid_ = -1;
    uint32_t run_bin_ = 0;
    uint64_t run_from_ = 0, target_from_, mapped_ = 0, unmapped_ = 0;
    int32_t seen_tid_ = -1, seen_pos_ = -1;
};

// Whether the file ends with BGZF's 28-byte marker block, as the reference looks for it before it reads anything
inline bool has_eof_marker(FILE *f)
{
    static const uint8_t marker[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t tail[28];
    const bool there = fseeko(f, -28, SEEK_END) == 0 && fread(tail, 1, 28, f) == 28 && memcmp(tail, marker, 28) == 0;
    fseeko(f, 0, SEEK_SET);
    return there;
}

// The BAM header read and passed over: the number of targets, or -1 (no BAM magic) / -2 (the header ends early)
inline int32_t skip_header(BgzfSeq &z)
{
    char magic[4];
    if (z.read(magic, 4) != 4 || memcmp(magic, "BAM\1", 4) != 0) return -1;
    std::vector<uint8_t> sink;
    auto pass = [&](int64_t n) { return sink.resize((size_t)n), z.read(sink.data(), n) == n; };
    int32_t l_text, n_ref;
    if (z.read(&l_text, 4) != 4 || l_text < 0 || !pass(l_text) || z.read(&n_ref, 4) != 4 || n_ref < 0) return -2;
    for (int32_t t = 0; t < n_ref; ++t) {
        int32_t l_name;
        if (z.read(&l_name, 4) != 4 || l_name < 0 || !pass((int64_t)l_name + 4)) return -2;
    }
    return n_ref;
}

// `samtools index`'s work over an open file.  kDone: `ix` is the index; kFailed: the reference gives up (its messages are in
// `err`, no index is written); kRefused: the reference's behaviour is undefined here (`err` says why, in the tool's own words).
// `err` also collects what the reference says on the way (no EOF marker, a truncated file).
inline int build(FILE *f, Index &ix, std::string &err)
{
    const char *gave_up = "[bam_index_build2] fail to index the BAM file.\n";
    if (!has_eof_marker(f)) err += "[bam_header_read] EOF marker is absent. The input is probably truncated.\n";
    BgzfSeq z(f);
    const int32_t n_ref = skip_header(z);
    if (n_ref == -1) {
        err += "[bam_header_read] invalid BAM binary header (this is not a BAM file).\n[bam_index_core] Invalid BAM header.";
        err += gave_up;
        return kFailed;
    }
    if (n_ref < 0) return err += "bam_index: the header ends early: outside the tool's domain\n", (int)kRefused;
    Indexer indexer(ix, n_ref, z.tell());
    Record r;
    int64_t status;
    bool unplaced_tail = false;
    for (uint64_t at = z.tell(); (status = read1(z, r)) >= 0; at = z.tell()) {
        const Indexer::Step step = indexer.add(r, at, z.tell());
        if (step == Indexer::kGoOn) continue;
        if (step == Indexer::kUnplacedFrom) {
            unplaced_tail = true;
            break;
        }
        err += indexer.said;
        if (step == Indexer::kUndefined) return kRefused;
        err += gave_up;
        return kFailed;
    }
    indexer.finish(z.tell());
    // behind the first record without a refID only such records may follow; they are counted, nothing else
    while (unplaced_tail && (status = read1(z, r)) >= 0) {
        ++ix.n_no_coor;
        if (r.tid >= 0) {
            err += "[bam_index_core] the alignment is not sorted: reads without coordinates prior to reads with coordinates.\n";
            err += gave_up;
            return kFailed;
        }
    }
    if (status < -1) {
        char line[96];
        snprintf(line, sizeof line, "[bam_index_core] truncated file? Continue anyway. (%d)\n", (int)status);
        err += line;
    }
    return kDone;
}

// `samtools index in.bam [out.index]` behind its argument check: what the reference prints is printed, the status is the
// reference's 0 whether or not an index was made, 2 where `build` refuses.  save_index writes an index that is already made (the
// device route's, or build's) to `out` or <in>.bai.
inline int save_index(const Index &ix, const char *in, const char *out)
{
    const std::string path = out ? std::string(out) : std::string(in) + ".bai";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) {
        fputs("[bam_index_build2] fail to create the index file.\n", stderr);
        return 0;
    }
    const bool ok = write_index(ix, f);
    if (fclose(f) != 0 || !ok) fprintf(stderr, "bam_index: writing %s failed\n", path.c_str());
    return 0;
}

inline int index_on_host(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb");
    if (!f) {
        fprintf(stderr, "open: %s\n", strerror(errno));
        fputs("[bam_index_build2] fail to open the BAM file.\n", stderr);
        return 0;
    }
    Index ix;
    std::string err;
    const int r = build(f, ix, err);
    fclose(f);
    fputs(err.c_str(), stderr);
    if (r == kRefused) return 2;
    if (r == kFailed) return 0;
    return save_index(ix, in, out);
}

}  // namespace bai
}  // namespace hpn
