// gzfastq_uniq -- drop-in for the reference tool of the same name (gzfastq_uniq.c): one record per distinct
// sequence of a plain or gzip FASTQ file (or per distinct pair of two files), with its multiplicity and the
// best-quality copy's name and quality; framing, grouping, ordering and formatting run on MI355X through libhpngs.
//
//   gzfastq_uniq -1 fq1 [-2 fq2] -o OUT [-h]
//
//   single-end  OUT_uniq.fq in the order the reference walks its hash table, OUT_sortKeyUniq.fq sorted by sequence
//   paired      OUT_1_uniq.fq and OUT_2_uniq.fq in the table's order
//   a record    "name\tcount\nsequence\n+\nquality\n"
//   stderr      the reference's lines: "unique reads number = ", "hash size: ", the two times; pairs: "error at N: NAME"
//               and "unmatched read name" at the first pair whose mate is missing or named otherwise -- reading stops
//               there and what was read is written, status 0.
//
// Where the reference has no answer -- a file that ends inside a record, a line of 1023+ characters, a damaged gzip
// stream, a quality line two or more bytes shorter than its sequence, no -o (it dies on its second output) -- this tool
// says so and leaves with status 2.  Names of more than two fields, on which the reference's unused split() overruns
// its array, are written like any other.  The reads are held in the memory of ONE device: an input beyond that is
// refused with the number of bytes that were needed.
#include <getopt.h>

#include <string>

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "gzfastq_uniq";

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s -1 fastq1 [-2 fastq2] -o OUT [-h]\n"
            "  Collapses duplicate reads of a plain or gzip FASTQ file: one record per distinct sequence\n"
            "  (with -2: per distinct pair of sequences), named and scored like its best-quality copy,\n"
            "  \"name<TAB>count\" on its first line (MI355X build of HighPerformanceNGS gzfastq_uniq).\n\n"
            "   [-1 fastq1] = fastq1.                                              [required]\n"
            "   [-2 fastq2] = fastq2, the mates of fastq1 in the same order.       [option]\n"
            "   [-o OUT]    = prefix of OUT_uniq.fq and OUT_sortKeyUniq.fq,\n"
            "                 with -2 of OUT_1_uniq.fq and OUT_2_uniq.fq.          [required]\n"
            "   [-h]        = This helpful help screen.                            [option]\n\n",
            prog);
    exit(1);
}

// one mate's `add` (host/store_tool.hpp)
static auto add_to(hpn_ctx *ctx, int mate)
{
    return [ctx, mate](const void *text, uint64_t n, bool last) {
        hpn_uniq_info ui = {};
        const int rc = hpn_fastq_uniq_add(ctx, mate, text, n, last, &ui);
        return chunk_taken(ctx, kTool, "hpn_fastq_uniq_add", rc, ui.irregular);
    };
}

// readNextNode (gzfastq_uniq.c:170-192) with the exact gzgets emulation: the gzeof test sits behind the FIRST gzgets only.
// The record goes out as canonical text -- the fields as strlen sees them, every line closed -- which the device frames like
// any regular chunk.  false: no record (gzeof).  Refuses what the reference crashes on.
struct HostReader {
    const char *path;
    InStream in;
    LineSource src;
    char name[kLineBuf], seq[kLineBuf], plus[kLineBuf], qual[kLineBuf];
    explicit HostReader(const char *p) : path(p), in(open_input_stream(p)), src(in) {}

    bool next(std::string &text)
    {
        size_t n1 = 0, n2 = 0, n3 = 0, n4 = 0;
        char *first = src.gets(name, kLineBuf, &n1);
        if (in.damaged()) refuse(kTool, path, kWhyDamaged);
        if (src.eof()) return false;
        if (!first || !src.gets(seq, kLineBuf, &n2) || !src.gets(plus, kLineBuf, &n3) || !src.gets(qual, kLineBuf, &n4)) {
            if (in.damaged()) refuse(kTool, path, kWhyDamaged);
            refuse(kTool, path, "the file ends inside a record");
        }
        if (name[n1 - 1] != '\n' || seq[n2 - 1] != '\n' || plus[n3 - 1] != '\n' || (n4 == (size_t)kLineBuf - 1 && qual[n4 - 1] != '\n'))
            refuse(kTool, path, "line of 1023 or more characters");
        const size_t l1 = strlen(name), l2 = strlen(seq), l4 = strlen(qual);
        if (!l1 || !l2 || !l4) refuse(kTool, path, "line that starts with a NUL byte");
        name[l1 - 1] = 0, seq[l2 - 1] = 0, qual[l4 - 1] = 0;   // :174, :179, :185
        if (l4 + 1 < l2) refuse(kTool, path, "quality line two or more bytes shorter than its sequence");
        text.append(name, l1 - 1).append("\n").append(seq, l2 - 1).append("\n+\n").append(qual, l4 - 1).append("\n");
        return true;
    }
};

struct HostError {
    bool any = false;
    uint64_t at = 0;
    std::string name;
};

static void host_feed(hpn_ctx *ctx, const char *read1, const char *read2, HostError &err)
{
    HostReader r1(read1);
    std::string t1, t2;
    auto flush = [&](int mate, std::string &t, bool last) {
        if (!add_to(ctx, mate)(t.data(), t.size(), last)) refuse(kTool, mate ? read2 : read1, kWhyTooShort);
        t.clear();
    };
    const size_t kFlush = (size_t)8 << 20;
    uint64_t n = 0;
    if (!read2) {
        while (r1.next(t1))
            if (t1.size() >= kFlush) flush(0, t1, false);
        flush(0, t1, true);
        return;
    }
    HostReader r2(read2);
    for (;; ++n) {
        const size_t before = t1.size(), before2 = t2.size();
        if (!r1.next(t1)) break;
        const bool have2 = r2.next(t2);
        // strncmp(name1, name2, strchr(name1, ' ') - name1): without a space the count is huge -- the names as wholes
        const char *sp = strchr(r1.name, ' ');
        if (!have2 || (sp ? strncmp(r1.name, r2.name, (size_t)(sp - r1.name)) : strcmp(r1.name, r2.name)) != 0) {
            err.any = true, err.at = n, err.name = r1.name;
            t1.resize(before), t2.resize(before2);   // the pair is not keyed
            break;
        }
        if (t1.size() >= kFlush) flush(0, t1, false), flush(1, t2, false);
    }
    flush(0, t1, true);
    flush(1, t2, true);
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *read1 = nullptr, *read2 = nullptr, *outfile = nullptr;
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "1:2:o:h?")) != -1) {
        switch (opt) {
        case '1': read1 = optarg; break;
        case '2': read2 = optarg; break;
        case 'o': outfile = optarg; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    if (!read1) {
        fprintf(stderr, "gzfastq_uniq: -1 fastq1 is required\n");
        return 2;
    }
    if (!outfile || outfile[0] == '-' || !outfile[0]) {
        fprintf(stderr, "gzfastq_uniq: -o OUT is required and cannot be standard output (the reference has no answer there: it closes its first output and dies on the second)\n");
        return 2;
    }
    for (const char *f : {read1, read2})
        if (f && access(f, R_OK) != 0) {
            fprintf(stderr, "open file %s failed\n", f);
            return 2;
        }
    hpn_ctx *ctx = open_tool_ctx();
    int rc;
    const long long begin = usec();

    bool done = false;
    HostError herr;
    if (text_path_enabled()) {
        if ((rc = hpn_fastq_uniq_begin(ctx, read2 != nullptr, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniq_begin");
        done = device_feed(ctx, kTool, read1, add_to(ctx, 0)) && (!read2 || device_feed(ctx, kTool, read2, add_to(ctx, 1)));
    }
    if (!done) {
        if ((rc = hpn_fastq_uniq_begin(ctx, read2 != nullptr, 0, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniq_begin");
        host_feed(ctx, read1, read2, herr);
    }
    const long long fed = usec();
    static hpn_uniq_result res;
    if ((rc = hpn_fastq_uniq_finish(ctx, &res)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_uniq_finish");
    if (herr.any) fprintf(stderr, "error at %ld: %s\nunmatched read name\n", (long)herr.at, herr.name.c_str());
    else if (res.unmatched >= 0) fprintf(stderr, "error at %ld: %s\nunmatched read name\n", (long)res.unmatched, res.unmatched_name);
    const unsigned long U = (unsigned long)res.n_unique, N = (unsigned long)res.n_records;
    fprintf(stderr, "unique reads number = %lu(%lu / %lu = %.3f%%)\n", U, U, N, 100.0 * U / N);
    fprintf(stderr, "hash size: %ld\n", (long)res.hash_size);
    fprintf(stderr, "Finished load hash at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    const long long grouped = usec();
    auto write_output = [&](int which, int mate, const char *suffix) {
        write_device_output(ctx, kTool, outfile, suffix, res.out_bytes[mate], text_slice_bytes((uint64_t)32 << 20),
                            [&](uint64_t at, void *buf, uint64_t cap, uint64_t *got) {
                                const int wrc = hpn_fastq_uniq_write(ctx, which, mate, at, buf, cap, got);
                                if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_fastq_uniq_write");
                            });
    };
    if (read2) {
        write_output(HPN_UNIQ_TABLE_ORDER, 0, "_1_uniq.fq");
        write_output(HPN_UNIQ_TABLE_ORDER, 1, "_2_uniq.fq");
    } else {
        write_output(HPN_UNIQ_TABLE_ORDER, 0, "_uniq.fq");
        write_output(HPN_UNIQ_KEY_ORDER, 0, "_sortKeyUniq.fq");
    }
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] uniq: reading and keying %.3f s, grouping and ordering %.3f s, formatting and writing %.3f s; %llu hash clashes\n",
                (double)(fed - begin) / 1e6, (double)(grouped - fed) / 1e6, (double)(usec() - grouped) / 1e6, (unsigned long long)res.hash_clashes);
    fprintf(stderr, "Finished  at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
