// gzfastq_sort -- drop-in for the reference tool of the same name (gzfastq_sort.c): the records of a plain or gzip FASTQ file
// (or of standard input) in ascending order of their name line or their sequence line -- first by the line's length, then by
// its bytes as unsigned, equal keys in input order; framing, ordering and formatting run on MI355X through libhpngs.
//
//   gzfastq_sort [-i FILE] [-o PREFIX] [-r N] [-s|-n] [-h]
//
//   -i        default "-": standard input.   -o  PREFIX_sort_by_seq.fq / PREFIX_sort_by_name.fq; a prefix that begins with '-'
//             (the default) means standard output.   -s / -n  by sequence (default) / by name; the last one given wins.
//   -r N      the reference's array size.  Without it the reference counts the reads first ("total_reads_num: ",
//             "max_reads_num: " on stderr) and rewinds -- which a pipe cannot do: the output is then EMPTY, here too.
//   a record  "name\nsequence\n+\nquality\n"
//   stderr    the reference's lines: the two counts (without -r), "name: a\tseq: b", three "done ... at T s".
//
// Where the reference has no answer -- a file that ends inside a record, a line of 1023+ characters, a damaged gzip stream,
// a -r below the number of reads (it writes behind its array) -- this tool says so and leaves with status 2.  The reads are
// held in the memory of ONE device: an input beyond that is refused with the number of bytes that were needed.
#include <getopt.h>

#include <string>

#include "../host/fastq_reader.hpp"
#include "../host/report.hpp"
#include "../host/text_feed.hpp"

using namespace hpn;

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s [-i Infile] [-o OUTFILE] [-r reads_count] [-s|-n] [-h]\n"
            "  Sorts the reads of a plain or gzip FASTQ file by sequence or by name: shorter lines first, lines of one\n"
            "  length by their bytes, equal ones in input order (MI355X build of HighPerformanceNGS gzfastq_sort).\n"
            "Example1:\n  zcat reads.fastq.gz | %s -r 8000000 -o out -s\n\n"
            "   [-i Infile] = Infile, default standard input.                    [option]\n"
            "   [-o OUTPUT] = prefix of OUTPUT_sort_by_seq.fq / _sort_by_name.fq,\n"
            "                 default (or a leading '-') standard output.        [option]\n"
            "   [-r reads_num] = an upper bound of the number of reads; needed\n"
            "                 when the input is a pipe.                          [option]\n"
            "   [-s ] sort by sequence (default).                                [option]\n"
            "   [-n ] sort by sequence name.                                     [option]\n"
            "   [-h] This helpful help screen.                                   [option]\n\n",
            prog, prog);
    exit(1);
}

[[noreturn]] static void refuse(const char *path, const char *why)
{
    fprintf(stderr, "gzfastq_sort: %s: %s (the reference has no answer there)\n", path, why);
    leave(2);
}

// str2unsigned_long (gzfastq_sort.c:71-83): the leading digits, modulo 2^64
static unsigned long parse_reads_num(const char *str)
{
    unsigned long v = 0;
    if (*str == '-') {
        fprintf(stderr, "reads count must be a positive integer!\n");
        exit(1);
    }
    for (; *str >= '0' && *str <= '9'; ++str) v = v * 10 + (unsigned long)(*str - '0');
    return v;
}

static bool add_chunk(hpn_ctx *ctx, const void *text, uint64_t n, bool last, uint64_t *records)
{
    hpn_sort_info si;
    const int rc = hpn_fastq_sort_add(ctx, text, n, last, &si);
    if (rc == HPN_E_CAPACITY) {
        fprintf(stderr, "gzfastq_sort: the reads do not fit into this device's memory: %s\n", hpn_ctx_last_error(ctx));
        leave(2);
    }
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_add");
    *records += si.n_records;
    return si.irregular == 0;
}

// The file's text into the session: the sink of feed_fastq_file (host/text_feed.hpp)
struct FileSink {
    hpn_ctx *ctx;
    uint64_t *records;
    void route_begins() {}
    bool start_over() { return false; }   // the session is void: the caller begins a new one
    bool chunk(const void *text, uint64_t n, bool last) { return add_chunk(ctx, text, n, last, records); }
};

// A file into the session on the device.  false: the text is not regular (or a route gave up half way) -- the session is void
// and the caller frames the file on the host.
static bool device_feed(hpn_ctx *ctx, const char *path, uint64_t *records)
{
    FileSink sink{ctx, records};
    const FeedEnd end = feed_fastq_file(ctx, path, "gzfastq_sort", sink);
    if (end == FeedEnd::kDamaged) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
    return end == FeedEnd::kDone;
}

// the whole inflated stream in memory (standard input, which cannot be read twice; a file whose text is not regular)
static void slurp(const char *path, std::string &mem)
{
    InStream in = open_input_stream(path);
    std::vector<char> buf((size_t)1 << 20);
    for (;;) {
        const int k = in.read(buf.data(), (unsigned)buf.size());
        if (k <= 0) break;
        mem.append(buf.data(), (size_t)k);
    }
    const bool damaged = in.damaged();
    in.close();
    if (damaged) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
}

// gzgets(file, buf, 1024) and gzeof over the stream in memory
struct MemLines {
    const std::string &d;
    size_t pos = 0;
    bool past = false;
    explicit MemLines(const std::string &s) : d(s) {}
    bool gets(const char **p, size_t *n)
    {
        if (pos >= d.size()) {
            past = true;
            return false;
        }
        const size_t room = d.size() - pos < (size_t)kLineBuf - 1 ? d.size() - pos : (size_t)kLineBuf - 1;
        const void *nl = memchr(d.data() + pos, '\n', room);
        size_t k = nl ? (size_t)((const char *)nl - (d.data() + pos)) + 1 : room;
        if (!nl && pos + k == d.size() && k < (size_t)kLineBuf - 1) past = true;
        *p = d.data() + pos, *n = k;
        pos += k;
        return true;
    }
};

// count_read (gzfastq_sort.c:185-198)
static unsigned long count_reads(const std::string &mem)
{
    MemLines in(mem);
    const char *p;
    size_t n;
    unsigned long reads = 0;
    while (in.gets(&p, &n)) {
        in.gets(&p, &n), in.gets(&p, &n), in.gets(&p, &n);
        ++reads;
    }
    return reads;
}

// readNextNode (gzfastq_sort.c:143-165) over the stream in memory: the gzeof test sits behind the FIRST gzgets only.  The
// records go out as canonical text -- the fields as strlen sees them, every line closed -- which the device frames like any
// regular chunk.  Refuses what the reference crashes on.
static void host_feed(hpn_ctx *ctx, const char *path, const std::string &mem, uint64_t *records)
{
    MemLines in(mem);
    std::string text;
    const size_t kFlush = (size_t)8 << 20;
    auto field = [&](bool have, const char *p, size_t n) {   // what strlen sees, without its last byte
        if (!have) refuse(path, "the file ends inside a record");
        if (n == (size_t)kLineBuf - 1 && p[n - 1] != '\n') refuse(path, "line of 1023 or more characters");
        const size_t l = strnlen(p, n);
        if (!l) refuse(path, "line that starts with a NUL byte");
        text.append(p, l - 1).push_back('\n');
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
            if (!add_chunk(ctx, text.data(), text.size(), false, records)) refuse(path, "records too short for the device's line index");
            text.clear();
        }
    }
    if (!add_chunk(ctx, text.data(), text.size(), true, records)) refuse(path, "records too short for the device's line index");
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *infile = "-", *outfile = "-";
    int by_name = 0, by_seq = 0;
    unsigned long reads_num = 0;
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "i:o:r:nsh?")) != -1) {
        switch (opt) {
        case 'i': infile = optarg; break;
        case 'o': outfile = optarg; break;
        case 'r': reads_num = parse_reads_num(optarg); break;
        case 'n': by_name = 1, by_seq = 0; break;
        case 's': by_name = 0, by_seq = 1; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    if (!by_name && !by_seq) by_seq = 1;
    const bool is_stdin = strncmp(infile, "-", 1) == 0 || !strcmp(infile, "");
    const bool rewindable = !is_stdin || lseek(STDIN_FILENO, 0, SEEK_CUR) != (off_t)-1;   // (gzrewind on a pipe fails)
    hpn_ctx *ctx = open_tool_ctx();
    int rc;
    const long long begin = usec();

    std::string mem;
    uint64_t records = 0;
    bool done = false, counted = false;
    unsigned long total_reads = 0;
    if (is_stdin) slurp(infile, mem);
    if (!reads_num && !rewindable) {   // the count consumed the pipe: the reference then reads nothing
        total_reads = count_reads(mem), counted = true;
        mem.clear();
    }
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_sort_begin(ctx, by_name, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_begin");
        if (is_stdin) {
            const uint64_t piece = text_chunk_bytes();
            uint64_t at = 0;
            do {
                const uint64_t k = mem.size() - at < piece ? mem.size() - at : piece;
                done = add_chunk(ctx, mem.data() + at, k, at + k == mem.size(), &records);
                at += k;
            } while (done && at < mem.size());
        } else {
            done = device_feed(ctx, infile, &records);
        }
    }
    if (!done) {
        if (!is_stdin) slurp(infile, mem);
        if (!reads_num && !counted) total_reads = count_reads(mem), counted = true;
        records = 0;
        if ((rc = hpn_fastq_sort_begin(ctx, by_name, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_begin");
        host_feed(ctx, infile, mem, &records);
    }
    if (reads_num && reads_num < records) {
        fprintf(stderr, "gzfastq_sort: -r %lu is below the file's %llu reads (the reference has no answer there: it writes behind its array)\n", reads_num,
                (unsigned long long)records);
        leave(2);
    }
    const long long fed = usec();
    static hpn_sort_result res;
    if ((rc = hpn_fastq_sort_finish(ctx, &res)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_finish");
    if (!reads_num) {
        if (!counted) total_reads = (unsigned long)res.n_records + res.lone_line;   // regular text: one gzgets group per record, one more for a lone last line
        fprintf(stderr, "total_reads_num: %ld\n", (long)total_reads);
        fprintf(stderr, "max_reads_num: %ld\n", (long)total_reads);
    }
    fprintf(stderr, "name: %d\tseq: %d\n", by_name, by_seq);
    fprintf(stderr, "done read file at %.3f s\n", (double)(fed - begin) / CLOCKS_PER_SEC);
    const long long ordered = usec();
    fprintf(stderr, "done qsort file at %.3f s\n", (double)(ordered - begin) / CLOCKS_PER_SEC);
    write_device_output(ctx, "gzfastq_sort", outfile, by_name ? "_sort_by_name.fq" : "_sort_by_seq.fq", res.out_bytes, text_slice_bytes((uint64_t)32 << 20),
                        [&](uint64_t at, void *buf, uint64_t cap, uint64_t *got) {
                            const int wrc = hpn_fastq_sort_write(ctx, at, buf, cap, got);
                            if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_fastq_sort_write");
                        });
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] sort: reading and framing %.3f s, ordering and formatting %.3f s, writing %.3f s; %u rounds, %llu records refined\n",
                (double)(fed - begin) / 1e6, (double)(ordered - fed) / 1e6, (double)(usec() - ordered) / 1e6, res.rounds, (unsigned long long)res.refined);
    fprintf(stderr, "done write file at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
