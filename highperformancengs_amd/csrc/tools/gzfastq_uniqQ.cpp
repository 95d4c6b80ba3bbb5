// gzfastq_uniqQ -- drop-in for the reference tool of the same name (gzfastq_uniqQ.c): one group per distinct sequence of a
// plain or gzip FASTQ file (or of standard input), with its multiplicity, the name of the last copy read and the quality line
// of EVERY copy, last read first; framing, grouping, ordering and formatting run on MI355X through libhpngs.
//
//   gzfastq_uniqQ [-1 FILE] [-S | -C] [-o OUT] [-h]
//
//   -1        default "-": standard input (any name that begins with '-', and the empty one).
//   -S / -C   groups by sequence ascending (memcmp, then length; the default) / by count descending, equal counts in the
//             order in which the reference walks its hash table; the last one given wins.
//   -o        OUT_sortKeyUniq.fq; an OUT that begins with '-' (the default) means standard output.
//   a group   "name\tcount\nsequence\n+\n", then one "quality\n" per copy
//   stderr    the reference's lines: "unique reads number = ", "hash size: ", the two times.
//
// Where the reference has no answer -- a file that ends inside a record, a line of 1023+ characters, a damaged gzip stream --
// this tool says so and leaves with status 2; a NUL byte in a line likewise.  A quality line shorter than its
// sequence is written like any other (the reference's quality sum is never printed).  The reads are held in the memory of
// ONE device: an input beyond that is refused with the number of bytes that were needed.
#include <getopt.h>

#include <string>

#include "../host/fastq_reader.hpp"
#include "../host/mem_lines.hpp"
#include "../host/report.hpp"
#include "../host/text_feed.hpp"

using namespace hpn;

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s [-1 READ1] [-C | -S] [-o OUTFILE] [-h]\n"
            "  Collapses duplicate reads of a plain or gzip FASTQ file and keeps every copy's quality line: per distinct\n"
            "  sequence \"name<TAB>count\", the sequence, \"+\", then the quality lines of its copies, the last one read\n"
            "  first (MI355X build of HighPerformanceNGS gzfastq_uniqQ).\n\n"
            "   [-1 READ1]  = fastq file, default standard input.                  [option]\n"
            "   [-C ]       = sort by sequence count, greatest first.              [option]\n"
            "   [-S ]       = sort by sequence (default).                          [option]\n"
            "   [-o OUTPUT] = prefix of OUTPUT_sortKeyUniq.fq, default (or a\n"
            "                 leading '-') standard output.                        [option]\n"
            "   [-h]        = This helpful help screen.                            [option]\n\n",
            prog);
    exit(1);
}

[[noreturn]] static void refuse(const char *path, const char *why)
{
    fprintf(stderr, "gzfastq_uniqQ: %s: %s (the reference has no answer there)\n", path, why);
    leave(2);
}

static bool add_chunk(hpn_ctx *ctx, const void *text, uint64_t n, bool last)
{
    hpn_uniq_info ui;
    const int rc = hpn_fastq_uniqq_add(ctx, text, n, last, &ui);
    if (rc == HPN_E_CAPACITY) {
        fprintf(stderr, "gzfastq_uniqQ: the reads do not fit into this device's memory: %s\n", hpn_ctx_last_error(ctx));
        leave(2);
    }
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniqq_add");
    return ui.irregular == 0;
}

// The file's text into the session: the sink of feed_fastq_file (host/text_feed.hpp)
struct FileSink {
    hpn_ctx *ctx;
    void route_begins() {}
    bool start_over() { return false; }   // the session is void: the caller begins a new one
    bool chunk(const void *text, uint64_t n, bool last) { return add_chunk(ctx, text, n, last); }
};

// A file into the session on the device.  false: the text is not regular (or a route gave up half way) -- the session is void
// and the caller frames the file on the host.
static bool device_feed(hpn_ctx *ctx, const char *path)
{
    FileSink sink{ctx};
    const FeedEnd end = feed_fastq_file(ctx, path, "gzfastq_uniqQ", sink);
    if (end == FeedEnd::kDamaged) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
    return end == FeedEnd::kDone;
}

// the whole inflated stream in memory (standard input, which cannot be read twice; a file whose text is not regular)
static void slurp(const char *path, std::string &mem)
{
    if (!slurp_stream(path, mem)) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
}

// readNextNode (gzfastq_uniqQ.c:181-203) over the stream in memory: the gzeof test sits behind the FIRST gzgets only.  The
// records go out as canonical text -- every line without its last byte and closed -- which the device frames like any
// regular chunk.  Refuses what the reference crashes on.
static void host_feed(hpn_ctx *ctx, const char *path, const std::string &mem)
{
    MemLines in(mem);
    std::string text;
    const size_t kFlush = (size_t)8 << 20;
    auto field = [&](bool have, const char *p, size_t n) {   // the line without its last byte
        if (!have) refuse(path, "the file ends inside a record");
        if (n == (size_t)kLineBuf - 1 && p[n - 1] != '\n') refuse(path, "line of 1023 or more characters");
        if (memchr(p, 0, n)) refuse(path, "NUL byte in a line");
        text.append(p, n - 1).push_back('\n');
    };
    for (;;) {
        const char *p;
        size_t n;
        bool have = in.gets(&p, &n);
        if (in.past) break;
        field(have, p, n);
        have = in.gets(&p, &n);
        field(have, p, n);
        if (!in.gets(&p, &n)) refuse(path, "the file ends inside a record");
        text.append("+\n");
        have = in.gets(&p, &n);
        field(have, p, n);
        if (text.size() >= kFlush) {
            if (!add_chunk(ctx, text.data(), text.size(), false)) refuse(path, "records too short for the device's line index");
            text.clear();
        }
    }
    if (!add_chunk(ctx, text.data(), text.size(), true)) refuse(path, "records too short for the device's line index");
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *read1 = "-", *outfile = "-";
    int by_count = 0;
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "1:o:CSh?")) != -1) {
        switch (opt) {
        case '1': read1 = optarg; break;
        case 'S': by_count = 0; break;
        case 'C': by_count = 1; break;
        case 'o': outfile = optarg; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    const bool is_stdin = strncmp(read1, "-", 1) == 0 || !strcmp(read1, "");
    if (!is_stdin && access(read1, R_OK) != 0) {
        fprintf(stderr, "open file %s failed\n", read1);
        return 2;
    }
    hpn_ctx *ctx = open_tool_ctx();
    int rc;
    const long long begin = usec();

    std::string mem;
    bool done = false;
    if (is_stdin) slurp(read1, mem);
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_uniqq_begin(ctx, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniqq_begin");
        if (is_stdin) {
            const uint64_t piece = text_chunk_bytes();
            uint64_t at = 0;
            do {
                const uint64_t k = mem.size() - at < piece ? mem.size() - at : piece;
                done = add_chunk(ctx, mem.data() + at, k, at + k == mem.size());
                at += k;
            } while (done && at < mem.size());
        } else {
            done = device_feed(ctx, read1);
        }
    }
    if (!done) {
        if (!is_stdin) slurp(read1, mem);
        if ((rc = hpn_fastq_uniqq_begin(ctx, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniqq_begin");
        host_feed(ctx, read1, mem);
    }
    const long long fed = usec();
    static hpn_uniqq_result res;
    if ((rc = hpn_fastq_uniqq_finish(ctx, &res)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniqq_finish");
    const unsigned long U = (unsigned long)res.n_unique, N = (unsigned long)res.n_records;
    fprintf(stderr, "unique reads number = %lu(%lu / %lu = %.3f%%)\n", U, U, N, 100.0 * U / N);
    fprintf(stderr, "hash size: %ld\n", (long)res.hash_size);
    fprintf(stderr, "Finished load hash at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    const long long grouped = usec();
    const int which = by_count ? HPN_UNIQQ_COUNT_ORDER : HPN_UNIQQ_KEY_ORDER;
    write_device_output(ctx, "gzfastq_uniqQ", outfile, "_sortKeyUniq.fq", res.out_bytes, text_slice_bytes((uint64_t)32 << 20),
                        [&](uint64_t at, void *buf, uint64_t cap, uint64_t *got) {
                            const int wrc = hpn_fastq_uniqq_write(ctx, which, at, buf, cap, got);
                            if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_fastq_uniqq_write");
                        });
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] uniqQ: reading and keying %.3f s, grouping and ordering %.3f s, formatting and writing %.3f s; %llu hash clashes, largest group %u\n",
                (double)(fed - begin) / 1e6, (double)(grouped - fed) / 1e6, (double)(usec() - grouped) / 1e6, (unsigned long long)res.hash_clashes,
                res.max_count);
    fprintf(stderr, "Finished  at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
