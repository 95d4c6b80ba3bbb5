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

#include "../host/bam_gpu.hpp"
#include "../host/fastq_reader.hpp"
#include "../host/gz_gpu.hpp"
#include "../host/tally_stream.hpp"
#include "../host/text_stream.hpp"
#include "../host/report.hpp"

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

static uint64_t slice_bytes()
{
    uint64_t slice = (uint64_t)32 << 20;
    if (const char *e = test_env("HPN_TEXT_SLICE")) slice = (uint64_t)atoll(e) < 64 ? 64 : (uint64_t)atoll(e);
    return slice;
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

// A file into the session on the device, through the routes gzfastq_uniq takes.  false: the text is not regular (or a route
// gave up half way) -- the session is void and the caller frames the file on the host.
class DeviceFeed {
public:
    DeviceFeed(hpn_ctx *ctx, uint64_t *records) : ctx_(ctx), records_(records) {}

    bool run(const char *path)
    {
        if (bam_gpu_enabled() && !test_env("HPN_NO_BGZF") && is_bgzf_file(path)) {   // bgzip: the blocks are inflated on the GPU
            BgzfGpuStream gs;
            if (gs.open_text(ctx_, path)) {
                for (bool fin = false; !fin;) {
                    hpn_raw_info bi;
                    const int r = gs.next(&bi);
                    if (r < 0) return false;
                    fin = r == 0 || gs.at_eof();
                    if (!device_text(gs.d_raw(), r == 0 ? 0 : bi.n_records, fin)) return false;
                }
                return true;
            }
        }
        const char *want = getenv("HPN_GZ_GPU");
        const bool gz_on_gpu = gz_gpu_enabled() && (usable_cpus() <= 8 || (want && want[0] == '1') || test_env("HPN_GZ_GPU_FORCE"));
        if (gz_on_gpu && !test_env("HPN_NO_MGZ") && !test_env("HPN_NO_PGZ") && is_plain_gzip_file(path)) {   // gzip members inflated on the GPU in stretches
            GzGpuStream gs;
            const long cpus = usable_cpus();
            uint32_t per_call = 5120;
            (void)hpn_inflate_slots(ctx_, &per_call);
            const uint32_t slots = per_call;
            if (const char *e = test_env("HPN_GZ_BATCH")) per_call = (uint32_t)atol(e);
            size_t stretch = 0;
            struct stat sb;
            if (!test_env("HPN_GZ_STRETCH") && stat(path, &sb) == 0) {
                stretch = ((size_t)sb.st_size / 4 / slots + 65536) & ~(size_t)65535;
                stretch = stretch < ((size_t)256 << 10) ? (size_t)256 << 10 : stretch > ((size_t)1 << 20) ? (size_t)1 << 20 : stretch;
            }
            if (gs.open(ctx_, path, (int)(cpus < 1 ? 1 : cpus > 16 ? 16 : cpus), per_call < 1 ? 1 : per_call, stretch)) {
                for (bool fin = false; !fin;) {
                    uint64_t n = 0;
                    const int r = gs.next(&n);
                    if (r < 0) return false;
                    fin = r == 0 || gs.at_end();
                    if (!device_text(gs.d_text(), n, fin)) return false;
                }
                return true;
            }
        }
        // text read (and, where compressed, inflated) by the host's reader threads, framed on the device
        TextPump pump(ctx_, path, text_chunk_bytes());
        if (!pump.ok()) die_hpn(ctx_, HPN_E_NOMEM, "gzfastq_sort");
        TextPump::Chunk c;
        while (pump.next(c)) {
            const bool ok = add_chunk(ctx_, c.p, c.n, c.eof, records_);
            pump.recycle(c);
            if (!ok) return false;
        }
        if (pump.damaged()) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
        return true;
    }

private:
    // text on the device, in slices (each framed by one call)
    bool device_text(const uint8_t *d_text, uint64_t total, bool fin)
    {
        const uint64_t slice = slice_bytes();
        for (uint64_t at = 0; at < total || (fin && total == 0);) {
            const uint64_t k = total - at < slice ? total - at : slice;
            if (!add_chunk(ctx_, d_text + at, k, fin && at + k == total, records_)) return false;
            at += k;
            if (total == 0) break;
        }
        return true;
    }
    hpn_ctx *ctx_;
    uint64_t *records_;
};

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

static void write_output(hpn_ctx *ctx, uint64_t total, const char *prefix, const char *suffix)
{
    FILE *out = fcreat_outfile(prefix, suffix);
    if (!out) leave(2);
    const uint64_t slice = slice_bytes();
    {
        AsyncWriter w(ctx, out, slice);   // the writer's thread puts one slice into the file while the next one is fetched
        if (!w.ok()) die_hpn(ctx, HPN_E_NOMEM, "gzfastq_sort");
        for (uint64_t at = 0; at < total;) {
            int idx;
            void *buf = w.acquire(&idx);
            uint64_t got = 0;
            const int rc = hpn_fastq_sort_write(ctx, at, buf, slice, &got);
            if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_fastq_sort_write");
            w.submit(idx, got);
            if (!got) break;
            at += got;
        }
        w.finish();
        if (w.failed()) {
            fprintf(stderr, "gzfastq_sort: writing %s%s failed (%s)\n", prefix, suffix, errno ? strerror(errno) : "short write");
            leave(2);
        }
    }
    if (fclose(out) != 0) {
        fprintf(stderr, "gzfastq_sort: writing %s%s failed (%s)\n", prefix, suffix, strerror(errno));
        leave(2);
    }
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
    hpn_ctx *ctx = nullptr;
    int dev0 = 0;
    if (const char *d = getenv("HPN_DEVICE")) dev0 = atoi(d);
    int rc = hpn_ctx_create(dev0, &ctx);
    if (rc != HPN_OK) die_hpn(nullptr, rc, "hpn_ctx_create");
    bind_for_device(ctx);
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
            DeviceFeed feed(ctx, &records);
            done = feed.run(infile);
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
    write_output(ctx, res.out_bytes, outfile, by_name ? "_sort_by_name.fq" : "_sort_by_seq.fq");
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] sort: reading and framing %.3f s, ordering and formatting %.3f s, writing %.3f s; %u rounds, %llu records refined\n",
                (double)(fed - begin) / 1e6, (double)(ordered - fed) / 1e6, (double)(usec() - ordered) / 1e6, res.rounds, (unsigned long long)res.refined);
    fprintf(stderr, "done write file at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
