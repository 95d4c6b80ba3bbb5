// pick_pair -- drop-in for the reference tool of the same name (pick_pair.c): the two files of a paired run, after one of them
// has lost reads to a filter, split into the reads that still have a mate and those that do not; the pairing is proposed and
// verified on MI355X through libhpngs.
//
//   pick_pair -1 READ1 -2 READ2 [-o OUT] [-h]
//
//   -1, -2    plain or gzip FASTQ, opened as files ("-" is no standard input here).  -1 also sets OUT: give -o behind it.
//   output    OUT_1_PE.fq.gz, OUT_1_SE.fq.gz, OUT_2_PE.fq.gz, OUT_2_SE.fq.gz, all four always: "name\nsequence\n+\nquality line".
//   stderr    the reference's lines: "Finished load file at T s", "Finished  at T s".
//
// The reference walks the files against each other with one strncmp per step, up to the first space of READ1's name; the walk
// is no clean merge-join and this tool reproduces it as it is, mispairings included.  The device proposes a pairing (the
// identity, then a join over an ascending READ2) and verifies that the walk gives exactly that; where neither verifies, where the
// text is irregular (long lines, NUL bytes, a stream that ends inside a record) or an input is no regular file, the walk itself
// runs on the host over the streams in memory.  Where the reference crashes -- one file runs out in front of the other -- this
// tool says so and leaves with status 2 and no outputs.  The reads are held in the memory of ONE device: an input beyond that is
// refused with the number of bytes that were needed.
#include <getopt.h>
#include <sys/stat.h>

#include <string>

#include "../host/store_tool.hpp"

using namespace hpn;

static const char kTool[] = "pick_pair";

static const char *const kSuffix[4] = {"_1_PE.fq.gz", "_1_SE.fq.gz", "_2_PE.fq.gz", "_2_SE.fq.gz"};

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s [-1 READ1] [-2 READ2] [-o OUTFILE] [-h]\n"
            "  Splits the two FASTQ files of a paired run into the reads that still have a mate (OUTFILE_1_PE.fq.gz,\n"
            "  OUTFILE_2_PE.fq.gz) and those that do not (OUTFILE_1_SE.fq.gz, OUTFILE_2_SE.fq.gz)\n"
            "  (MI355X build of HighPerformanceNGS pick_pair).\n"
            "Example1:\n  %s -1 R1.clean.fastq -2 R2.clean.fastq -o pair_out\n\n"
            "   [-1 READ1]  = fastq formated file1; also sets OUTFILE.              [required]\n"
            "   [-2 READ2]  = fastq formated file2.                                [required]\n"
            "   [-o OUTPUT] = OUTPUT prefix, behind -1.                            [option]\n"
            "   [-h]        = This helpful help screen.                            [option]\n\n",
            prog, prog);
    exit(1);
}

// readNextNode (pick_pair.c) over a stream in memory: four gzgets into a 1024-byte buffer, gzeof tested behind the first; name and
// sequence lose their last byte, the third line is dropped, the quality line is kept as strdup sees it.
struct Reader {
    const char *path;
    MemLines in;
    std::string name, seq, qual;
    bool have = false;   // a record is held
    Reader(const char *p, const std::string &mem) : path(p), in(mem) {}
    void field(std::string &to, bool got, const char *p, size_t n)
    {
        if (!got) refuse(kTool, path, "the file ends inside a record");
        const size_t l = strnlen(p, n);
        if (!l) refuse(kTool, path, "line that starts with a NUL byte");
        to.assign(p, l - 1);
    }
    void next()
    {
        const char *p;
        size_t n;
        bool got = in.gets(&p, &n);
        if (in.past) {
            have = false;
            return;
        }
        field(name, got, p, n);
        got = in.gets(&p, &n);
        field(seq, got, p, n);
        (void)in.gets(&p, &n);
        if (!in.gets(&p, &n)) refuse(kTool, path, "the file ends inside a record");
        qual.assign(p, strnlen(p, n));
        have = true;
    }
    void emit(std::string &out)
    {
        out.append(name).push_back('\n');
        out.append(seq).append("\n+\n").append(qual);
    }
};

static int name_cmp(const Reader &a, const Reader &b)
{
    const size_t sp = a.name.find(' ');
    return strncmp(a.name.c_str(), b.name.c_str(), sp == std::string::npos ? (size_t)-1 : sp);   // (NULL - name: every byte and the NUL)
}

// load_fastq_file's loop as it is.  The NULL records it dereferences are refused.
static void host_walk(const char *read1, const char *read2, const std::string &mem1, const std::string &mem2, std::string out[4])
{
    Reader a(read1, mem1), b(read2, mem2);
    for (;;) {
        a.next();
        b.next();
        while (a.have) {
            if (!b.have) refuse(kTool, read2, "the file runs out in front of the other one");
            if (name_cmp(a, b) >= 0) break;
            a.emit(out[1]);
            a.next();
        }
        while (b.have) {
            if (!a.have) refuse(kTool, read1, "the file runs out in front of the other one");
            if (name_cmp(a, b) <= 0) break;
            b.emit(out[3]);
            b.next();
        }
        if (!a.have && !b.have) break;
        if (a.have) a.emit(out[0]);
        if (b.have) b.emit(out[2]);
    }
}

static bool regular_file(const char *path)
{
    struct stat sb;
    return stat(path, &sb) == 0 && S_ISREG(sb.st_mode);
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *read1 = nullptr, *read2 = nullptr, *outfile = "out";
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "1:2:o:h?")) != -1) {
        switch (opt) {
        case '1': read1 = optarg, outfile = optarg; break;   // (-1 sets the prefix as well: a -o in front of it is lost)
        case '2': read2 = optarg; break;
        case 'o': outfile = optarg; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    if (!read1 || !read2) {
        fprintf(stderr, "pick_pair: -1 READ1 and -2 READ2 are required (the reference opens a NULL name there)\n");
        return 2;
    }
    const long long begin = usec();
    for (const char *f : {read1, read2})
        if (access(f, R_OK) != 0) {
            fprintf(stderr, "open file %s failed\n", f);
            return 1;
        }
    hpn_ctx *ctx = open_tool_ctx();
    int rc;

    static hpn_pair_result res;
    const char *route = "host";
    bool done = false;
    if (text_path_enabled() && regular_file(read1) && regular_file(read2)) {
        if ((rc = hpn_fastq_pair_begin(ctx, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_pair_begin");
        auto add_to = [&](int mate) {
            return [ctx, mate](const void *text, uint64_t n, bool last) {
                hpn_sort_info si = {};
                const int arc = hpn_fastq_pair_add(ctx, mate, text, n, last, &si);
                return chunk_taken(ctx, kTool, "hpn_fastq_pair_add", arc, si.irregular);
            };
        };
        if (device_feed(ctx, kTool, read1, add_to(0)) && device_feed(ctx, kTool, read2, add_to(1))) {
            rc = hpn_fastq_pair_finish(ctx, &res);
            if (rc == HPN_OK) done = true, route = res.route == HPN_PAIR_IDENTITY ? "identity" : "join";
            else if (!(rc == HPN_E_DOMAIN && res.unverified)) die_hpn(ctx, rc, "hpn_fastq_pair_finish");
        }
    }
    std::string text[4];
    if (!done) {
        std::string mem1, mem2;
        slurp_or_refuse(kTool, read1, mem1);
        slurp_or_refuse(kTool, read2, mem2);
        host_walk(read1, read2, mem1, mem2, text);
    }
    const long long split = usec();
    const uint64_t slice = text_slice_bytes((uint64_t)32 << 20);
    void *buf = nullptr;
    if (done && hpn_host_malloc(ctx, slice, &buf) != HPN_OK) die_hpn(ctx, HPN_E_NOMEM, kTool);
    for (int w = 0; w < 4; ++w)   // from the session, or the host walk's text
        write_gz_output(kTool, std::string(outfile) + kSuffix[w], done ? nullptr : &text[w], res.out_bytes[w], buf, slice,
                        [&](uint64_t at, void *to, uint64_t cap, uint64_t *got) {
                            const int wrc = hpn_fastq_pair_write(ctx, w, at, to, cap, got);
                            if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_fastq_pair_write");
                        });
    if (buf) hpn_host_free(ctx, buf);
    fprintf(stderr, "Finished load file at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] pick_pair: route %s; reading and pairing %.3f s, deflating and writing %.3f s; %llu pairs, %llu + %llu singles\n", route,
                (double)(split - begin) / 1e6, (double)(usec() - split) / 1e6, (unsigned long long)res.n_pairs, (unsigned long long)res.n_single[0],
                (unsigned long long)res.n_single[1]);
    fprintf(stderr, "Finished  at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
