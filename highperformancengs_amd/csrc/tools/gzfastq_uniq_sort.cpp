// gzfastq_uniq_sort -- drop-in for the reference tool of the same name (gzfastq_uniq_sort.c): one record per distinct
// sequence of a plain or gzip FASTQ file (or per distinct pair of two files) with its multiplicity and the first copy's name
// and quality, most frequent first, as gzip files; framing, grouping, ordering and formatting run on MI355X through libhpngs.
//
//   gzfastq_uniq_sort -1 READ1 [-2 READ2] [-o OUT] [-h]
//
//   outputs     OUT_1_uniq.fq.gz and, with -2, OUT_2_uniq.fq.gz.  -1 also sets OUT to its own argument (gzfastq_uniq_sort.c:291):
//               a later -o wins, an earlier one is overwritten.  The gzip bytes are this tool's, the text inside is the
//               reference's.
//   a record    "name\tcount\nSEQ\n+\nquality\n"; SEQ of mate 1 is the first strLen bytes of the (joined) sequence, SEQ of
//               mate 2 what follows them, strLen = the length of the first READ1 sequence that is not empty.
//   order       count descending, equal counts in the order in which the reference walks its hash table.
//   stderr      the reference's lines, with this tool's times: the input names, "total_reads_num: ", "loaded N at T s",
//               pairs: "error at N: NAME" at the first pair whose mate is missing or named otherwise -- reading stops there and
//               what was read is written --, "unique reads number = ", "hash size: ", "total reads = ", the percentage, the
//               two times.
//
// Where the reference has no answer this tool says so and leaves with status 2 without an output file: fewer than ten reads
// (it divides by a tenth of their number), a file that ends inside a record or has one more line with its newline, a line of
// 1023+ characters, a NUL byte, a damaged gzip stream, a pair whose joined sequences have more than 1023 bytes or fewer than
// strLen.  The reads are held in the memory of ONE device: an input beyond that is refused with the bytes that were needed.
#include <getopt.h>

#include <string>

#include "../host/fastq_reader.hpp"
#include "../host/gz_writer.hpp"
#include "../host/mem_lines.hpp"
#include "../host/report.hpp"
#include "../host/text_feed.hpp"

using namespace hpn;

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s -1 READ1 [-2 READ2] [-o OUT] [-h]\n"
            "  Collapses duplicate reads of a plain or gzip FASTQ file: one record per distinct sequence (with -2: per\n"
            "  distinct pair of sequences), named and scored like its first copy, \"name<TAB>count\" on its first line,\n"
            "  the most frequent first (MI355X build of HighPerformanceNGS gzfastq_uniq_sort).\n\n"
            "   [-1 READ1]  = fastq file 1.                                        [required]\n"
            "   [-2 READ2]  = fastq file 2, the mates of READ1 in the same order.  [option]\n"
            "   [-o OUT]    = prefix of OUT_1_uniq.fq.gz (and OUT_2_uniq.fq.gz);\n"
            "                 default READ1, when given behind -1.                 [option]\n"
            "   [-h]        = This helpful help screen.                            [option]\n\n",
            prog);
    exit(1);
}

[[noreturn]] static void refuse(const char *path, const char *why)
{
    fprintf(stderr, "gzfastq_uniq_sort: %s: %s (the reference has no answer there)\n", path, why);
    leave(2);
}

static bool add_chunk(hpn_ctx *ctx, int mate, const void *text, uint64_t n, bool last)
{
    hpn_uniq_info ui;
    const int rc = hpn_fastq_usort_add(ctx, mate, text, n, last, &ui);
    if (rc == HPN_E_CAPACITY) {
        fprintf(stderr, "gzfastq_uniq_sort: the reads do not fit into this device's memory: %s\n", hpn_ctx_last_error(ctx));
        leave(2);
    }
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_add");
    return ui.irregular == 0;
}

// One mate's text into the session: the sink of feed_fastq_file (host/text_feed.hpp)
struct MateSink {
    hpn_ctx *ctx;
    int mate;
    void route_begins() {}
    bool start_over() { return false; }   // the session is void: the caller begins a new one
    bool chunk(const void *text, uint64_t n, bool last) { return add_chunk(ctx, mate, text, n, last); }
};

// One mate's file into the session on the device.  false: the text is not regular (or a route gave up half way) -- the session
// is void and the caller frames the files on the host.
static bool device_feed(hpn_ctx *ctx, int mate, const char *path)
{
    MateSink sink{ctx, mate};
    const FeedEnd end = feed_fastq_file(ctx, path, "gzfastq_uniq_sort", sink);
    if (end == FeedEnd::kDamaged) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
    return end == FeedEnd::kDone;
}

// the whole inflated stream in memory
static void slurp(const char *path, std::string &mem)
{
    if (!slurp_stream(path, mem)) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
}

// readNextNode (gzfastq_uniq_sort.c:67-88) over one mate's stream in memory: the gzeof test sits behind the FIRST gzgets only.
// The records go out as canonical text -- every line without its last byte and closed -- which the device frames like any
// regular chunk; one open line behind the last record, which count_read counts, stays as it is.  Refuses what the reference
// crashes on.
static void host_feed(hpn_ctx *ctx, int mate, const char *path)
{
    std::string mem;
    slurp(path, mem);
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
        if (in.past) {
            if (have) {
                if (memchr(p, 0, n)) refuse(path, "NUL byte in a line");
                text.append(p, n);
            }
            break;
        }
        field(have, p, n);
        have = in.gets(&p, &n);
        field(have, p, n);
        if (!in.gets(&p, &n)) refuse(path, "the file ends inside a record");
        text.append("+\n");
        have = in.gets(&p, &n);
        field(have, p, n);
        if (text.size() >= kFlush) {
            if (!add_chunk(ctx, mate, text.data(), text.size(), false)) refuse(path, "records too short for the device's line index");
            text.clear();
        }
    }
    if (!add_chunk(ctx, mate, text.data(), text.size(), true)) refuse(path, "records too short for the device's line index");
}

// One mate's output through GzWriter.  The file is made here, behind hpn_fastq_usort_finish: a refusal leaves none.
static double write_output(hpn_ctx *ctx, int mate, const std::string &path, uint64_t total)
{
    GzWriter w(path.c_str());
    if (!w.ok()) {
        fprintf(stderr, "open file %s failed\n", path.c_str());
        leave(2);
    }
    const uint64_t slice = text_slice_bytes((uint64_t)32 << 20);
    void *buf = nullptr;
    if (hpn_host_malloc(ctx, slice, &buf) != HPN_OK) die_hpn(ctx, HPN_E_NOMEM, "gzfastq_uniq_sort");
    for (uint64_t at = 0; at < total;) {
        uint64_t got = 0;
        const int rc = hpn_fastq_usort_write(ctx, mate, at, buf, slice, &got);
        if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_write");
        if (!got) break;
        if (!w.write(buf, got)) break;
        at += got;
    }
    if (!w.finish()) {
        fprintf(stderr, "gzfastq_uniq_sort: writing %s failed (%s)\n", path.c_str(), errno ? strerror(errno) : "short write");
        unlink(path.c_str());
        leave(2);
    }
    hpn_host_free(ctx, buf);
    return w.deflate_seconds();
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *read1 = nullptr, *read2 = nullptr, *outfile = "out";
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "1:2:o:h?")) != -1) {
        switch (opt) {
        case '1': read1 = optarg, outfile = optarg; break;   // (:289-293)
        case '2': read2 = optarg; break;
        case 'o': outfile = optarg; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    if (!read1) {
        fprintf(stderr, "gzfastq_uniq_sort: -1 READ1 is required\n");
        return 2;
    }
    const long long begin = usec();
    fprintf(stderr, "%s", read1);   // (:315-320)
    if (read2) fprintf(stderr, "\t%s\n", read2);
    else fprintf(stderr, "\n");
    for (const char *f : {read1, read2})
        if (f && access(f, R_OK) != 0) {
            fprintf(stderr, "open file %s failed\n", f);
            return 2;
        }
    hpn_ctx *ctx = open_tool_ctx();
    int rc;

    bool done = false;
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_usort_begin(ctx, read2 != nullptr, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_begin");
        done = device_feed(ctx, 0, read1) && (!read2 || device_feed(ctx, 1, read2));
    }
    if (!done) {
        if ((rc = hpn_fastq_usort_begin(ctx, read2 != nullptr, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_begin");
        host_feed(ctx, 0, read1);
        if (read2) host_feed(ctx, 1, read2);
    }
    const long long fed = usec();
    static hpn_usort_result res;
    rc = hpn_fastq_usort_finish(ctx, &res);
    if (rc == HPN_E_DOMAIN && res.no_answer) refuse(read2 && res.no_answer != HPN_USORT_FEW_READS ? read2 : read1, hpn_ctx_last_error(ctx));
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_finish");
    const unsigned long U = (unsigned long)res.n_unique, N = (unsigned long)res.n_records, e = (unsigned long)res.table_reads;
    const double now = (double)(usec() - begin) / CLOCKS_PER_SEC;
    fprintf(stderr, "total_reads_num: %ld\n", (long)e);   // (:183)
    if (N)   // (e >= 10: the session refuses fewer)
        for (unsigned long n = e / 10; n <= N; n += e / 10) fprintf(stderr, "loaded %lu at %.3f s\n", n, now);   // (:161-163)
    if (res.unmatched >= 0) fprintf(stderr, "error at %ld: %s\n", (long)res.unmatched, res.unmatched_name);      // (:138)
    fprintf(stderr, "unique reads number = %d\n", (int)U);
    fprintf(stderr, "Finished load hash at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    fprintf(stderr, "hash size: %ld\ntotal reads = %ld\n", (unsigned long)res.hash_size, N);
    fprintf(stderr, "unique reads percentage: %.3f%%\n", (float)U / N * 100);
    const long long grouped = usec();
    double deflate_s = write_output(ctx, 0, std::string(outfile) + "_1_uniq.fq.gz", res.out_bytes[0]);
    if (read2) deflate_s += write_output(ctx, 1, std::string(outfile) + "_2_uniq.fq.gz", res.out_bytes[1]);
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] uniq_sort: reading and keying %.3f s, grouping and ordering %.3f s, formatting, deflating and writing %.3f s (%.3f s of deflate over the threads); %llu hash clashes, largest group %u\n",
                (double)(fed - begin) / 1e6, (double)(grouped - fed) / 1e6, (double)(usec() - grouped) / 1e6, deflate_s,
                (unsigned long long)res.hash_clashes, res.max_count);
    fprintf(stderr, "Finished  at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
