// gzfastq_mrle -- drop-in for the reference tool of the same name (gzfastq_mrle.c): the quality lines of a plain or gzip FASTQ file
// (or of standard input) run-length packed by its two-pass codec over the symbols # / 7 < B F, and decoded again; framing, codec
// and the layout of the output streams run on MI355X through libhpngs.
//
//   gzfastq_mrle [-i FILE] [-o PREFIX] [-s|-n] [-h]
//
//   -i        default "-": standard input.   -o  PREFIX_sort_by_seq.fq / PREFIX_sort_by_name.fq; a prefix that begins with '-'
//             (the default) means standard output.   -s / -n  choose that NAME only (the last one given wins): nothing is sorted,
//             the records stay in input order.
//   output    the packed file: per record one byte (uint8_t)size and the size encoded bytes -- a flag byte (bit s: the runs of
//             symbol s are escaped), then literals and run tokens (symbol, 0xFF per 255, the rest - 1).  Standard output: per
//             record what the decoder makes of those bytes, and '\n'.  With a '-' prefix the reference writes BOTH through two
//             stdio streams on descriptor 1 and closes the packed one first: blocks of 4,096 bytes of either stream in the order
//             their buffers overflow, then the packed stream's remainder; the text's remainder is lost.  This tool writes the
//             same bytes.
//   stderr    the reference's lines: "name: a\tseq: b", "done read file at T s", "list count: N", four more "done ... at T s".
//
// Where the reference has no answer -- a file that ends inside a record, a line of 1023+ characters, a damaged gzip stream, a
// quality byte outside the six (it indexes an 8-entry table at 255) -- this tool says so and leaves with status 2.  The reads are
// held in the memory of ONE device: an input beyond that is refused with the number of bytes that were needed.
#include <getopt.h>

#include <string>

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "gzfastq_mrle";

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s [-i Infile] [-o OUTFILE] [-s|-n] [-h]\n"
            "  Run-length packs the quality lines (symbols # / 7 < B F) of a plain or gzip FASTQ file, the reads in input order,\n"
            "  and prints the decoded lines (MI355X build of HighPerformanceNGS gzfastq_mrle).\n"
            "Example1:\n  zcat reads.fastq.gz | %s -o out > decoded.txt\n\n"
            "   [-i Infile] = Infile, default standard input.                    [option]\n"
            "   [-o OUTPUT] = prefix of OUTPUT_sort_by_seq.fq / _sort_by_name.fq,\n"
            "                 default (or a leading '-') standard output.        [option]\n"
            "   [-s ] name the output _sort_by_seq.fq (default).                 [option]\n"
            "   [-n ] name the output _sort_by_name.fq.                          [option]\n"
            "   [-h] This helpful help screen.                                   [option]\n\n",
            prog, prog);
    exit(1);
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *infile = "-", *outfile = "-";
    int by_name = 0, by_seq = 0;
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "i:o:nsh?")) != -1) {
        switch (opt) {
        case 'i': infile = optarg; break;
        case 'o': outfile = optarg; break;
        case 'n': by_name = 1, by_seq = 0; break;
        case 's': by_name = 0, by_seq = 1; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    if (!by_name && !by_seq) by_seq = 1;
    const bool is_stdin = strncmp(infile, "-", 1) == 0 || !strcmp(infile, "");
    const bool shared = outfile[0] == '-' || !outfile[0];   // the packed file IS standard output
    hpn_ctx *ctx = open_tool_ctx();
    int rc;
    const long long begin = usec();

    std::string mem;
    uint64_t records = 0;
    bool done = false;
    auto add = [&](const void *text, uint64_t n, bool last) {
        hpn_sort_info si = {};
        const int arc = hpn_mrle_add(ctx, text, n, last, &si);
        records += si.n_records;
        return chunk_taken(ctx, kTool, "hpn_mrle_add", arc, si.irregular);
    };
    if (is_stdin) slurp_or_refuse(kTool, infile, mem);
    if (text_path_enabled()) {
        if ((rc = hpn_mrle_begin(ctx, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_mrle_begin");
        done = is_stdin ? memory_feed(mem, add) : device_feed(ctx, kTool, infile, add);
    }
    if (!done) {
        if (!is_stdin) slurp_or_refuse(kTool, infile, mem);
        records = 0;
        if ((rc = hpn_mrle_begin(ctx, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_mrle_begin");
        // readNextNode (gzfastq_mrle.c, the same as gzfastq_sort.c:143-165): the fields as strlen sees them
        if (const char *why = canonical_feed(mem, FieldRule::kStrlen, false, add)) refuse(kTool, infile, why);
    }
    const long long fed = usec();
    static hpn_mrle_result res;
    rc = hpn_mrle_finish(ctx, &res);
    if (rc == HPN_E_DOMAIN && res.bad_record >= 0) {
        fprintf(stderr, "gzfastq_mrle: %s: quality byte outside #/7<BF in record %lld (the reference has no answer there)\n", infile, (long long)res.bad_record);
        leave(2);
    }
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_mrle_finish");
    const long long packed = usec();
    fprintf(stderr, "name: %d\tseq: %d\n", by_name, by_seq);
    fprintf(stderr, "done read file at %.3f s\nlist count: %d\n", (double)(fed - begin) / CLOCKS_PER_SEC, (int)res.n_records);
    fprintf(stderr, "done dump_array at %.3f s\n", (double)(packed - begin) / CLOCKS_PER_SEC);
    fprintf(stderr, "done sort file at %.3f s\n", (double)(packed - begin) / CLOCKS_PER_SEC);
    auto put = [&](int which, const char *prefix, const char *suffix) {
        write_device_output(ctx, kTool, prefix, suffix, res.out_bytes[which], text_slice_bytes((uint64_t)32 << 20),
                            [&](uint64_t at, void *buf, uint64_t cap, uint64_t *got) {
                                const int wrc = hpn_mrle_write(ctx, which, at, buf, cap, got);
                                if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_mrle_write");
                            });
    };
    if (shared) {
        put(HPN_MRLE_SHARED, "-", "");
    } else {
        put(HPN_MRLE_PACKED, outfile, by_name ? "_sort_by_name.fq" : "_sort_by_seq.fq");
        put(HPN_MRLE_TEXT, "-", "");
    }
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] mrle: reading and framing %.3f s, coding %.3f s, writing %.3f s; packed %llu, text %llu, shared %llu bytes\n",
                (double)(fed - begin) / 1e6, (double)(packed - fed) / 1e6, (double)(usec() - packed) / 1e6, (unsigned long long)res.out_bytes[HPN_MRLE_PACKED],
                (unsigned long long)res.out_bytes[HPN_MRLE_TEXT], (unsigned long long)res.out_bytes[HPN_MRLE_SHARED]);
    fprintf(stderr, "done write file at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    fprintf(stderr, "done free list at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
