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

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "gzfastq_uniqQ";

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
    auto add = [&](const void *text, uint64_t n, bool last) {
        hpn_uniq_info ui = {};
        const int arc = hpn_fastq_uniqq_add(ctx, text, n, last, &ui);
        return chunk_taken(ctx, kTool, "hpn_fastq_uniqq_add", arc, ui.irregular);
    };
    if (is_stdin) slurp_or_refuse(kTool, read1, mem);
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_uniqq_begin(ctx, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniqq_begin");
        done = is_stdin ? memory_feed(mem, add) : device_feed(ctx, kTool, read1, add);
    }
    if (!done) {
        if (!is_stdin) slurp_or_refuse(kTool, read1, mem);
        if ((rc = hpn_fastq_uniqq_begin(ctx, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniqq_begin");
        // readNextNode (gzfastq_uniqQ.c:181-203): every line without its last byte
        if (const char *why = canonical_feed(mem, FieldRule::kLine, false, add)) refuse(kTool, read1, why);
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
    write_device_output(ctx, kTool, outfile, "_sortKeyUniq.fq", res.out_bytes, text_slice_bytes((uint64_t)32 << 20),
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
