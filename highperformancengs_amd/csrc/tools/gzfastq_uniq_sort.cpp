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

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "gzfastq_uniq_sort";

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

    const char *reads[2] = {read1, read2};
    auto add_to = [&](int mate) {
        return [ctx, mate](const void *text, uint64_t n, bool last) {
            hpn_uniq_info ui = {};
            const int arc = hpn_fastq_usort_add(ctx, mate, text, n, last, &ui);
            return chunk_taken(ctx, kTool, "hpn_fastq_usort_add", arc, ui.irregular);
        };
    };
    bool done = false;
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_usort_begin(ctx, read2 != nullptr, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_begin");
        done = device_feed(ctx, kTool, read1, add_to(0)) && (!read2 || device_feed(ctx, kTool, read2, add_to(1)));
    }
    if (!done) {
        if ((rc = hpn_fastq_usort_begin(ctx, read2 != nullptr, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_usort_begin");
        // readNextNode (gzfastq_uniq_sort.c:67-88): every line without its last byte; one open line behind the last record, which
        // count_read counts, stays as it is
        for (int mate = 0; mate < 2 && reads[mate]; ++mate) {
            std::string mem;
            slurp_or_refuse(kTool, reads[mate], mem);
            if (const char *why = canonical_feed(mem, FieldRule::kLine, true, add_to(mate))) refuse(kTool, reads[mate], why);
        }
    }
    const long long fed = usec();
    static hpn_usort_result res;
    rc = hpn_fastq_usort_finish(ctx, &res);
    if (rc == HPN_E_DOMAIN && res.no_answer) refuse(kTool, read2 && res.no_answer != HPN_USORT_FEW_READS ? read2 : read1, hpn_ctx_last_error(ctx));
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
    const uint64_t slice = text_slice_bytes((uint64_t)32 << 20);
    void *buf = nullptr;
    if (hpn_host_malloc(ctx, slice, &buf) != HPN_OK) die_hpn(ctx, HPN_E_NOMEM, kTool);
    double deflate_s = 0;
    for (int mate = 0; mate < 2 && reads[mate]; ++mate)
        deflate_s += write_gz_output(kTool, std::string(outfile) + (mate ? "_2_uniq.fq.gz" : "_1_uniq.fq.gz"), nullptr, res.out_bytes[mate], buf, slice,
                                     [&](uint64_t at, void *to, uint64_t cap, uint64_t *got) {
                                         const int wrc = hpn_fastq_usort_write(ctx, mate, at, to, cap, got);
                                         if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_fastq_usort_write");
                                     });
    hpn_host_free(ctx, buf);
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] uniq_sort: reading and keying %.3f s, grouping and ordering %.3f s, formatting, deflating and writing %.3f s (%.3f s of deflate over the threads); %llu hash clashes, largest group %u\n",
                (double)(fed - begin) / 1e6, (double)(grouped - fed) / 1e6, (double)(usec() - grouped) / 1e6, deflate_s,
                (unsigned long long)res.hash_clashes, res.max_count);
    fprintf(stderr, "Finished  at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
