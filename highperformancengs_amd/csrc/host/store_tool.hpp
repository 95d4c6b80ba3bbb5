// store_tool.hpp -- what the tools over a store session share (gzfastq_uniq, gzfastq_uniqQ, gzfastq_uniq_sort, gzfastq_sort,
// fastq2twobit, pick_pair, gzfastq_mrle, rfastqc_tally): the refusal, the outcome of an *_add call, a file or a stream in memory into the session, the host's
// framing of text the device refused, and a device output through GzWriter.  A tool hands in its `add`: a callable
// bool(const void *text, uint64_t n, bool last) around its family's *_add, false when the chunk was not regular.
#pragma once
#include "gz_writer.hpp"
#include "mem_lines.hpp"
#include "report.hpp"
#include "text_feed.hpp"

namespace hpn {

constexpr const char *kWhyDamaged = "damaged gzip stream (CRC-32 / ISIZE / data error)";
constexpr const char *kWhyTooShort = "records too short for the device's line index";

[[noreturn]] inline void refuse(const char *tool, const char *path, const char *why)
{
    fprintf(stderr, "%s: %s: %s (the reference has no answer there)\n", tool, path, why);
    leave(2);
}

// What an *_add call (`what`) returned: beyond the device's memory and any other error end the tool; true: the chunk was regular
inline bool chunk_taken(hpn_ctx *ctx, const char *tool, const char *what, int rc, uint32_t irregular)
{
    if (rc == HPN_E_CAPACITY) {
        fprintf(stderr, "%s: the reads do not fit into this device's memory: %s\n", tool, hpn_ctx_last_error(ctx));
        leave(2);
    }
    if (rc != HPN_OK) die_hpn(ctx, rc, what);
    return irregular == 0;
}

// the sink of feed_fastq_file (text_feed.hpp) over an `add`
template <class Add>
struct StoreSink {
    Add &add;
    void route_begins() {}
    bool start_over() { return false; }   // the session is void: the caller begins a new one
    bool chunk(const void *text, uint64_t n, bool last) { return add(text, n, last); }
};

// A file into the session on the device.  false: the text is not regular (or a route gave up half way) -- the session is void
// and the caller frames the file on the host.
template <class Add>
bool device_feed(hpn_ctx *ctx, const char *tool, const char *path, Add add)
{
    StoreSink<Add> sink{add};
    const FeedEnd end = feed_fastq_file(ctx, path, tool, sink);
    if (end == FeedEnd::kDamaged) refuse(tool, path, kWhyDamaged);
    return end == FeedEnd::kDone;
}

// the whole inflated stream in memory (standard input, which cannot be read twice; a file whose text is not regular)
inline void slurp_or_refuse(const char *tool, const char *path, std::string &mem)
{
    if (!slurp_stream(path, mem)) refuse(tool, path, kWhyDamaged);
}

// a stream in memory into the session as it is, in the pieces a file would come in; false: the text is not regular
template <class Add>
bool memory_feed(const std::string &mem, Add add)
{
    const uint64_t piece = text_chunk_bytes();
    uint64_t at = 0;
    bool ok;
    do {
        const uint64_t k = mem.size() - at < piece ? mem.size() - at : piece;
        ok = add(mem.data() + at, k, at + k == mem.size());
        at += k;
    } while (ok && at < mem.size());
    return ok;
}

// What a field of a record is.  kStrlen: what strlen sees in gzgets' buffer, without its last byte -- a line that starts with a
// NUL byte is refused (gzfastq_sort.c, fastq2twobit.c).  kLine: the line without its last byte -- a NUL byte anywhere is refused
// (gzfastq_uniqQ.c, gzfastq_uniq_sort.c).
enum class FieldRule { kStrlen, kLine };

// readNextNode over a stream in memory (four gzgets into a 1024-byte buffer, the gzeof test behind the FIRST only) into the
// session as canonical text -- name, sequence and quality by `rule`, every line closed, the third line "+" -- which the device
// frames like any regular chunk, `flush` bytes or more at a time.  keep_lone_line: one open line behind the last record, which
// count_read counts, goes along as it is.  Returns why the reference has no answer for this text, or nullptr.
template <class Add>
const char *canonical_feed(const std::string &mem, FieldRule rule, bool keep_lone_line, Add add, size_t flush = (size_t)8 << 20)
{
    MemLines in(mem);
    std::string text;
    auto field = [&](bool have, const char *p, size_t n) -> const char * {
        if (!have) return "the file ends inside a record";
        if (n == (size_t)kLineBuf - 1 && p[n - 1] != '\n') return "line of 1023 or more characters";
        if (rule == FieldRule::kLine) {
            if (memchr(p, 0, n)) return "NUL byte in a line";
        } else if (!(n = strnlen(p, n))) {
            return "line that starts with a NUL byte";
        }
        text.append(p, n - 1).push_back('\n');
        return nullptr;
    };
    for (;;) {
        const char *p, *why;
        size_t n;
        bool have = in.gets(&p, &n);
        if (in.past) {
            if (have && keep_lone_line) {
                if (rule == FieldRule::kLine ? memchr(p, 0, n) != nullptr : !p[0]) return rule == FieldRule::kLine ? "NUL byte in a line" : "line that starts with a NUL byte";
                text.append(p, rule == FieldRule::kLine ? n : strnlen(p, n));
            }
            break;
        }
        if ((why = field(have, p, n))) return why;
        have = in.gets(&p, &n);
        if ((why = field(have, p, n))) return why;
        if (!in.gets(&p, &n)) return "the file ends inside a record";
        text.append("+\n");
        have = in.gets(&p, &n);
        if ((why = field(have, p, n))) return why;
        if (text.size() >= flush) {
            if (!add(text.data(), text.size(), false)) return kWhyTooShort;
            text.clear();
        }
    }
    return add(text.data(), text.size(), true) ? nullptr : kWhyTooShort;
}

// One output through GzWriter: `text` where the host made it, else the `total` bytes that fetch(at, buf, slice, &got) copies from
// the device (and dies itself where the ABI refuses).  The file is made here, behind the session's _finish: a refusal leaves
// none.  Returns the seconds of deflate, summed over the writer's threads.
template <class Fetch>
double write_gz_output(const char *tool, const std::string &path, const std::string *text, uint64_t total, void *buf, uint64_t slice, Fetch fetch)
{
    GzWriter w(path.c_str());
    if (!w.ok()) {
        fprintf(stderr, "open file %s failed\n", path.c_str());
        leave(2);
    }
    if (text) {
        if (!text->empty()) (void)w.write(text->data(), text->size());
    } else {
        for (uint64_t at = 0; at < total;) {
            uint64_t got = 0;
            fetch(at, buf, slice, &got);
            if (!got) break;
            if (!w.write(buf, got)) break;
            at += got;
        }
    }
    if (!w.finish()) {
        fprintf(stderr, "%s: writing %s failed (%s)\n", tool, path.c_str(), errno ? strerror(errno) : "short write");
        unlink(path.c_str());
        leave(2);
    }
    return w.deflate_seconds();
}

}  // namespace hpn
