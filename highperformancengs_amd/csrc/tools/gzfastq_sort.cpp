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

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "gzfastq_sort";

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
    auto add = [&](const void *text, uint64_t n, bool last) {
        hpn_sort_info si = {};
        const int arc = hpn_fastq_sort_add(ctx, text, n, last, &si);
        records += si.n_records;
        return chunk_taken(ctx, kTool, "hpn_fastq_sort_add", arc, si.irregular);
    };
    if (is_stdin) slurp_or_refuse(kTool, infile, mem);
    if (!reads_num && !rewindable) {   // the count consumed the pipe: the reference then reads nothing
        total_reads = count_reads(mem), counted = true;
        mem.clear();
    }
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_sort_begin(ctx, by_name, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_begin");
        done = is_stdin ? memory_feed(mem, add) : device_feed(ctx, kTool, infile, add);
    }
    if (!done) {
        if (!is_stdin) slurp_or_refuse(kTool, infile, mem);
        if (!reads_num && !counted) total_reads = count_reads(mem), counted = true;
        records = 0;
        if ((rc = hpn_fastq_sort_begin(ctx, by_name, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_begin");
        // readNextNode (gzfastq_sort.c:143-165): the fields as strlen sees them
        if (const char *why = canonical_feed(mem, FieldRule::kStrlen, false, add)) refuse(kTool, infile, why);
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
    write_device_output(ctx, kTool, outfile, by_name ? "_sort_by_name.fq" : "_sort_by_seq.fq", res.out_bytes, text_slice_bytes((uint64_t)32 << 20),
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
