// rfastqc_tally -- the one call behind the reference's Rfastqc.R, qsort_hash_count(fq1, fq2) of its R plugin (Rgzfastq_uniq.c),
// as a command-line tool: the reference has no command line for it, so this one is ours.  Framing, the tallies and the duplicate
// counts run on MI355X through libhpngs (hpn_rfastqc_*).
//
//   rfastqc_tally -1 FQ1 [-2 FQ2] -o PREFIX [-h]
//
//   -1, -2    plain or gzip FASTQ, opened as files.  With -2 the files are read pair by pair, ordinal by ordinal; records of FQ2
//             behind FQ1's last are never read, as in the plugin.
//   output    the list's elements as raw little-endian arrays, for R's readBin:
//               PREFIX.dup.i32             int[unique]    the count of every distinct key, descending (list element 1)
//               PREFIX.R1.gc.f64           double[reads]  GC fraction per read                        (2)
//               PREFIX.R1.quality.i32      int[128*300]   Quality[q + 128 pos]                        (3)
//               PREFIX.R1.nucleotide.i32   int[5*300]     Nucleotide[5 pos + code]                    (4)
//               PREFIX.R1.length.i32       int[300]       Length[L - 1]                               (5)
//             and the four PREFIX.R2.* files with -2 (6 .. 9).
//   stderr    the plugin's lines: "mean GC% = ..", "hash size: ..", "unique reads U (U/N= P% )", "Finished load hash at T s",
//             "Finished at T s".  The mean is the sequential sum of the returned gc vector, as the plugin sums it; the hash size is
//             the closed form of its table's growth (13,400,000, then 2 size + 1 whenever the count has reached 0.75 size at an
//             insert).
//
// Where the plugin has no answer -- a sequence length outside 1..300, a quality line beyond 300, a byte >= 128, FQ2 shorter than
// FQ1, a file that ends inside a record, a line of 1023+ characters, a damaged gzip stream -- this tool says so and leaves with
// status 2 and no outputs.  The reads are held in the memory of ONE device: an input beyond that is refused with the number of
// bytes that were needed.
#include <getopt.h>

#include <string>
#include <vector>

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "rfastqc_tally";

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s -1 FQ1 [-2 FQ2] -o PREFIX [-h]\n"
            "  The list Rfastqc.R plots -- duplicate counts, per-read GC, the Quality and Nucleotide matrices, the length\n"
            "  histogram -- of one FASTQ file or of a pair, as raw arrays PREFIX.dup.i32, PREFIX.R1.gc.f64, PREFIX.R1.quality.i32,\n"
            "  PREFIX.R1.nucleotide.i32, PREFIX.R1.length.i32 (and PREFIX.R2.*)\n"
            "  (MI355X build of HighPerformanceNGS Rgzfastq_uniq qsort_hash_count).\n"
            "Example1:\n  %s -1 R1.fastq.gz -2 R2.fastq.gz -o sample\n\n"
            "   [-1 FQ1]    = fastq formated file1, plain or gzip.                 [required]\n"
            "   [-2 FQ2]    = fastq formated file2: the mates of file1.            [option]\n"
            "   [-o PREFIX] = prefix of the output files.                          [required]\n"
            "   [-h]        = This helpful help screen.                            [option]\n\n",
            prog, prog);
    exit(1);
}

// the size of the plugin's table behind U inserts (hashtbl.c: the growth test comes in front of every insert)
static unsigned long table_size(uint64_t U)
{
    unsigned long size = 13400000ul;   // (HSIZE)ELECNT * 1.34
    while (U && (double)(U - 1) >= size * 0.75) size = size * 2 + 1;
    return size;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *fq[2] = {nullptr, nullptr}, *prefix = nullptr;
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "1:2:o:h")) != -1) {
        switch (opt) {
        case '1': fq[0] = optarg; break;
        case '2': fq[1] = optarg; break;
        case 'o': prefix = optarg; break;
        default: usage(argv[0]); break;
        }
    }
    if (!fq[0] || !prefix || optind < argc) usage(argv[0]);
    const int mates = fq[1] ? 2 : 1;
    const long long begin = usec();
    for (int k = 0; k < mates; ++k)
        if (access(fq[k], R_OK) != 0) {
            fprintf(stderr, "open file %s failed\n", fq[k]);
            return 1;
        }
    hpn_ctx *ctx = open_tool_ctx();
    int rc;

    auto add_to = [&](int mate) {
        return [ctx, mate](const void *text, uint64_t n, bool last) {
            hpn_sort_info si = {};
            const int arc = hpn_rfastqc_add(ctx, mate, text, n, last, &si);
            return chunk_taken(ctx, kTool, "hpn_rfastqc_add", arc, si.irregular);
        };
    };
    bool done = false;
    if (text_path_enabled()) {
        if ((rc = hpn_rfastqc_begin(ctx, mates > 1, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_rfastqc_begin");
        done = device_feed(ctx, kTool, fq[0], add_to(0)) && (mates < 2 || device_feed(ctx, kTool, fq[1], add_to(1)));
    }
    if (!done) {   // readNextNode (Rgzfastq_uniq.c:122-138) on the host: the fields as strlen sees them
        if ((rc = hpn_rfastqc_begin(ctx, mates > 1, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_rfastqc_begin");
        for (int k = 0; k < mates; ++k) {
            std::string mem;
            slurp_or_refuse(kTool, fq[k], mem);
            if (const char *why = canonical_feed(mem, FieldRule::kStrlen, false, add_to(k))) refuse(kTool, fq[k], why);
        }
    }
    const long long fed = usec();
    static hpn_rfastqc_result res;
    rc = hpn_rfastqc_finish(ctx, &res);
    if (rc == HPN_E_DOMAIN && res.bad_record >= 0) {
        fprintf(stderr, "%s: %s: %s (the reference has no answer there)\n", kTool, fq[res.bad_mate], hpn_ctx_last_error(ctx));
        leave(2);
    }
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_rfastqc_finish");
    const long long tallied = usec();

    const uint64_t slice = (uint64_t)4 << 20;   // elements
    void *buf = nullptr;
    if (hpn_host_malloc(ctx, slice * 8, &buf) != HPN_OK) die_hpn(ctx, HPN_E_NOMEM, kTool);
    double total_gc = 0;
    auto put = [&](int which, int mate, const std::string &name, bool sum) {
        const size_t es = which == HPN_RFASTQC_GC ? 8 : 4;
        FILE *f = fopen(name.c_str(), "wb");
        if (!f) {
            fprintf(stderr, "open file %s failed\n", name.c_str());
            leave(2);
        }
        for (uint64_t at = 0;;) {
            uint64_t got = 0;
            const int wrc = hpn_rfastqc_read(ctx, which, mate, at, buf, slice, &got);
            if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_rfastqc_read");
            if (!got) break;
            if (sum)
                for (uint64_t i = 0; i < got; ++i) total_gc += ((const double *)buf)[i];   // in input order, one after the other
            if (fwrite(buf, es, got, f) != got) {
                fprintf(stderr, "%s: writing %s failed (%s)\n", kTool, name.c_str(), strerror(errno));
                unlink(name.c_str());
                leave(2);
            }
            at += got;
        }
        if (fclose(f) != 0) {
            fprintf(stderr, "%s: writing %s failed (%s)\n", kTool, name.c_str(), strerror(errno));
            unlink(name.c_str());
            leave(2);
        }
    };
    const std::string p(prefix);
    put(HPN_RFASTQC_DUP, 0, p + ".dup.i32", false);
    for (int k = 0; k < mates; ++k) {
        const std::string r = p + (k ? ".R2" : ".R1");
        put(HPN_RFASTQC_GC, k, r + ".gc.f64", k == 0);
        put(HPN_RFASTQC_QUALITY, k, r + ".quality.i32", false);
        put(HPN_RFASTQC_NUCLEOTIDE, k, r + ".nucleotide.i32", false);
        put(HPN_RFASTQC_LENGTH, k, r + ".length.i32", false);
    }
    hpn_host_free(ctx, buf);
    const unsigned long n = (unsigned long)res.n_records;
    fprintf(stderr, "mean GC%% = %f%%\n", (double)total_gc / n * 100);
    fprintf(stderr, "hash size: %ld\n", table_size(res.n_unique));
    fprintf(stderr, "unique reads %d (%d/%ld= %.3f%% )\n", (int)res.n_unique, (int)res.n_unique, n, (double)res.n_unique / n * 100);
    fprintf(stderr, "Finished load hash at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] rfastqc_tally: reading and framing %.3f s, tallying and grouping %.3f s, writing %.3f s; %llu reads, %llu keys, %llu clashes\n",
                (double)(fed - begin) / 1e6, (double)(tallied - fed) / 1e6, (double)(usec() - tallied) / 1e6, (unsigned long long)res.n_records,
                (unsigned long long)res.n_unique, (unsigned long long)res.hash_clashes);
    fprintf(stderr, "Finished at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
