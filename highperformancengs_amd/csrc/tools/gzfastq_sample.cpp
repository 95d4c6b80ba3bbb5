// gzfastq_sample -- drop-in for the reference tool of the same name (gzfastq_sample.c): a subsample of the
// reads of a plain or gzip FASTQ file, framing, selection and formatting running on MI355X through libhpngs.
//
//   gzfastq_sample {-1 fq1} [-2 fq2] [-s SEED.FRAC] [-n N] [-q|-f] [-h]        (-o is accepted and ignored, as there)
//
//   -s SEED.FRAC  keep a record iff ((X31(name line) + seed) & 0xffffff) / 2^24 < FRAC; SEED != 0 goes through
//                 srand / rand first (:363-369, :150-153).  Output basename(fq).FRAC.gz ("%f") in the current directory.
//   -n N          count the records, draw N of them without replacement (Fisher-Yates driven by MT19937 seeded
//                 with 4357, :227-278), write them in file order.  Output basename(fq).N.gz.  N beyond the number of
//                 records: a message, the -1 output left as an empty file, exit status 0 -- as the reference leaves it.
//   -2 fq2        the mate file: record i is written exactly when record i of fq1 is.
//   -f            FASTA records (">name_i\nseq\n") instead of FASTQ ("name_i\nseq\n+\nquality").
//
// The output is a gzip file whose decompressed bytes are the reference's (host/gz_writer.hpp).  Where the
// reference crashes -- a file that ends inside a record, a line of 1023+ characters, a damaged gzip stream --
// this tool says so and leaves with status 2; what the output files hold then is unspecified.
// One device: an input is not spread over several GPUs (HPN_NGPU is not read).
#include <getopt.h>
#include <libgen.h>
#include <math.h>

#include <algorithm>
#include <string>

#include "../host/fastq_reader.hpp"
#include "../host/gz_writer.hpp"
#include "../host/report.hpp"
#include "../host/text_feed.hpp"

using namespace hpn;

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s {-1 fastq1} [-2 fastq2] [-s FLOAT] [-n UL] [-q|-f] [-h]\n"
            "  Writes a subsample of the reads of a plain or gzip FASTQ file\n"
            "  (MI355X build of HighPerformanceNGS gzfastq_sample).\n\n"
            "   [-1 fastq1] = fastq1.                                                           [required]\n"
            "   [-2 fastq2] = fastq2.                                                           [option]\n"
            "   [-s FLOAT]  = fraction of templates to subsample; integer part as seed.         [option]\n"
            "   [-n UL]     = number of picked reads.                                           [option]\n"
            "   [-f ]       = output fasta format.                                              [option]\n"
            "   [-q ]       = output fastq format[default].                                     [option]\n"
            "   [-h]        = This helpful help screen.                                         [option]\n\n",
            prog);
    exit(1);
}

[[noreturn]] static void refuse(const char *path, const char *why)
{
    fprintf(stderr, "gzfastq_sample: %s: %s (the reference has no answer there: it crashes)\n", path, why);
    leave(2);
}

// MT19937 (Matsumoto & Nishimura 1998, with the seeding of 2002) and the reference's bounded draw: scale = 0xffffffff / k,
// words are drawn until word / scale < k.
struct Mt19937 {
    uint32_t mt[624];
    int at = 624;
    explicit Mt19937(uint32_t seed)
    {
        mt[0] = seed;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    }
    uint32_t word()
    {
        if (at == 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            at = 0;
        }
        uint32_t y = mt[at++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        return y ^ (y >> 18);
    }
    uint64_t below(uint64_t k)
    {
        const uint64_t scale = 0xffffffffull / k;
        if (!scale) {
            fprintf(stderr, "gzfastq_sample: more than 2^32 - 1 records: beyond the reference's generator\n");
            leave(2);
        }
        uint64_t r;
        do r = word() / scale;
        while (r >= k);
        return r;
    }
};

// index_without_replacement + qsort of the first `pick` entries (:176-199, :249)
static std::vector<uint64_t> draw_picks(uint64_t n, uint64_t pick)
{
    std::vector<uint64_t> xs(n);
    for (uint64_t i = 0; i < n; ++i) xs[i] = i;
    Mt19937 rng(4357);
    for (uint64_t i = n ? n - 1 : 0; i > 0; --i) std::swap(xs[rng.below(i + 1)], xs[i]);
    xs.resize(pick);
    std::sort(xs.begin(), xs.end());
    return xs;
}

[[noreturn]] static void write_failed()
{
    fprintf(stderr, "gzfastq_sample: writing the output failed (%s)\n", errno ? strerror(errno) : "short write");
    leave(2);
}

struct Pass {
    const hpn_sample_rule *rule = nullptr;   // nullptr: count_read -- records are counted, nothing is written
    GzWriter *out = nullptr;
    std::vector<uint64_t> *kept = nullptr;   // receives the ordinals of the kept records (the mate's pick list)
    uint64_t n_records = 0, n_kept = 0;
};

// One pass over a file on the device: the sink of feed_fastq_file (host/text_feed.hpp).
class DevicePass {
public:
    DevicePass(hpn_ctx *ctx, Pass &p) : ctx_(ctx), p_(p) {}
    ~DevicePass()
    {
        if (obuf_) hpn_host_free(ctx_, obuf_);
    }

    void route_begins()
    {
        const int rc = hpn_fastq_text_begin(ctx_);
        if (rc != HPN_OK) die_hpn(ctx_, rc, "gzfastq_sample");
    }
    bool start_over()
    {
        p_.n_records = p_.n_kept = 0;
        if (p_.kept) p_.kept->clear();
        return !p_.out || p_.out->restart();
    }
    // one chunk through the ABI; false: irregular text (or a sample that outgrew the buffer: records of a few bytes)
    bool chunk(const void *text, uint64_t n, bool last)
    {
        if (!p_.rule) {
            hpn_text_info ti;
            const int rc = hpn_fastq_text_records(ctx_, text, n, last, &ti);
            if (rc != HPN_OK) die_hpn(ctx_, rc, "hpn_fastq_text_records");
            if (ti.irregular) return false;
            p_.n_records += ti.n_records;
            return true;
        }
        const uint64_t need = 2 * n + 16384;
        if (need > ocap_) {
            if (obuf_) hpn_host_free(ctx_, obuf_);
            obuf_ = nullptr;
            if (hpn_host_malloc(ctx_, need, &obuf_) != HPN_OK) die_hpn(ctx_, HPN_E_NOMEM, "gzfastq_sample");
            ocap_ = need;
        }
        if (p_.kept && kbuf_.size() < (n + 8192) / 4) kbuf_.resize((n + 8192) / 4);
        hpn_sample_info si;
        const int rc = hpn_fastq_text_sample(ctx_, text, n, last, p_.rule, obuf_, ocap_, p_.kept ? kbuf_.data() : nullptr, kbuf_.size(), &si);
        if (rc == HPN_E_CAPACITY) return false;
        if (rc != HPN_OK) die_hpn(ctx_, rc, "hpn_fastq_text_sample");
        if (si.irregular) return false;
        p_.n_records += si.n_records;
        p_.n_kept += si.n_kept;
        if (p_.kept) p_.kept->insert(p_.kept->end(), kbuf_.begin(), kbuf_.begin() + (ptrdiff_t)si.n_kept);
        if (!p_.out->write(obuf_, si.n_bytes)) write_failed();
        return true;
    }

private:
    hpn_ctx *ctx_;
    Pass &p_;
    void *obuf_ = nullptr;
    uint64_t ocap_ = 0;
    std::vector<uint64_t> kbuf_;
};

// The same pass framed on the host with the exact gzgets emulation (readNextNode, :315-335), the selection made here
// from the same rule.  Refuses what the reference crashes on.
static void host_pass(const char *path, Pass &p)
{
    p.n_records = p.n_kept = 0;
    if (p.kept) p.kept->clear();
    if (p.out && !p.out->restart()) {
        fprintf(stderr, "gzfastq_sample: cannot rewind the output\n");
        leave(2);
    }
    InStream in = open_input_stream(path);
    LineSource src(in);
    const hpn_sample_rule *r = p.rule;
    std::string obuf;
    char name[kLineBuf], seq[kLineBuf], plus[kLineBuf], qual[kLineBuf];
    uint64_t at_pick = 0;
    for (;;) {
        size_t n1 = 0, n2 = 0, n3 = 0, n4 = 0;
        if (!src.gets(name, kLineBuf, &n1)) break;
        if (src.eof() || !src.gets(seq, kLineBuf, &n2) || !src.gets(plus, kLineBuf, &n3) || !src.gets(qual, kLineBuf, &n4)) {
            if (in.damaged()) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
            refuse(path, "the file ends inside a record");
        }
        if (name[n1 - 1] != '\n' || seq[n2 - 1] != '\n' || plus[n3 - 1] != '\n' || (n4 == (size_t)kLineBuf - 1 && qual[n4 - 1] != '\n'))
            refuse(path, "line of 1023 or more characters");
        const size_t l1 = strlen(name), l2 = strlen(seq);
        if (!l1 || !l2) refuse(path, "line that starts with a NUL byte");
        name[l1 - 1] = 0, seq[l2 - 1] = 0;   // :319, :323
        const uint64_t g = r ? r->first_ordinal + p.n_records : p.n_records;
        ++p.n_records;
        if (!r) continue;
        bool keep;
        if (r->mode == HPN_SAMPLE_FRACTION) {
            uint32_t h = (uint32_t)(int32_t)(signed char)name[0];   // khash.h:336-341
            if (h)
                for (const char *s = name + 1; *s; ++s) h = (h << 5) - h + (uint32_t)(int32_t)(signed char)*s;
            keep = ((h + r->seed_add) & 0xffffffu) < r->threshold;
        } else {
            while (at_pick < r->n_picks && r->picks[at_pick] < g) ++at_pick;
            keep = at_pick < r->n_picks && r->picks[at_pick] == g;
        }
        if (!keep) continue;
        ++p.n_kept;
        if (p.kept) p.kept->push_back(g);
        char tag[32];
        snprintf(tag, sizeof tag, "_%llu\n", (unsigned long long)(g + 1));
        if (r->fasta) obuf.append(">").append(name).append(tag).append(seq).append("\n");
        else obuf.append(name).append(tag).append(seq).append("\n+\n").append(qual);
        if (obuf.size() >= ((size_t)8 << 20)) {
            if (!p.out->write(obuf.data(), obuf.size())) refuse(path, "writing the output failed");
            obuf.clear();
        }
    }
    if (in.damaged()) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
    if (p.out && !p.out->write(obuf.data(), obuf.size())) refuse(path, "writing the output failed");
    in.close();
}

static void run_pass(hpn_ctx *ctx, const char *path, Pass &p)
{
    // kIrregular: the text is not regular (or a route gave up half way and the output could not be rewound) -- nothing of the
    // pass counts and the file is framed on the host
    FeedEnd end = FeedEnd::kIrregular;
    if (text_path_enabled()) {
        DevicePass d(ctx, p);
        end = feed_fastq_file(ctx, path, "gzfastq_sample", d);
    }
    if (end == FeedEnd::kDamaged) refuse(path, "damaged gzip stream (CRC-32 / ISIZE / data error)");
    if (end == FeedEnd::kIrregular) host_pass(path, p);
}

static std::string out_name(const char *in, const char *mid)
{
    std::string copy(in);
    return std::string(basename(&copy[0])) + "." + mid + ".gz";
}

static GzWriter *create_out(const std::string &name)
{
    GzWriter *w = new GzWriter(name.c_str());
    if (!w->ok()) {
        fprintf(stderr, "open file %s failed\n", name.c_str());
        leave(2);
    }
    return w;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *read1 = nullptr, *read2 = nullptr;
    unsigned long reads_n = 0;
    uint32_t seed = 0;
    double frac = -1.;
    bool fasta = false;
    if (argc < 2) usage(argv[0]);
    int opt;
    char *q;
    while ((opt = getopt(argc, argv, "1:2:o:s:n:qfh?")) != -1) {
        switch (opt) {
        case '1': read1 = optarg; break;
        case '2': read2 = optarg; break;
        case 'o': break;
        case 's':
            if ((seed = (uint32_t)strtol(optarg, &q, 10)) != 0) {   // :363-369
                srand(seed);
                seed = (uint32_t)rand();
            }
            frac = strtod(q, &q);
            break;
        case 'n': reads_n = strtoul(optarg, NULL, 10); break;
        case 'f': fasta = true; break;
        case 'q': fasta = false; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    if (!read1) {
        fprintf(stderr, "gzfastq_sample: -1 fastq1 is required\n");
        return 2;
    }
    for (const char *f : {read1, read2})
        if (f && access(f, R_OK) != 0) {
            fprintf(stderr, "open file %s failed\n", f);
            return 2;
        }
    hpn_ctx *ctx = open_tool_ctx();
    const long long begin = usec();
    double t_deflate = 0, t_waited = 0;
    int gz_threads = 0;

    if (frac > 0) {   // proportion_file, :280-313
        char mid[64];
        snprintf(mid, sizeof mid, "%f", frac);
        GzWriter *o1 = create_out(out_name(read1, mid));
        GzWriter *o2 = read2 ? create_out(out_name(read2, mid)) : nullptr;
        const double scaled = frac * 16777216.0;   // exact; (k & 0xffffff) / 2^24 < frac  <=>  (k & 0xffffff) < ceil(frac * 2^24)
        hpn_sample_rule rule = {};
        rule.mode = HPN_SAMPLE_FRACTION, rule.fasta = fasta, rule.seed_add = seed;
        rule.threshold = scaled >= 16777216.0 ? 1u << 24 : (uint32_t)ceil(scaled);
        std::vector<uint64_t> kept;
        Pass p1;
        p1.rule = &rule, p1.out = o1, p1.kept = read2 ? &kept : nullptr;
        run_pass(ctx, read1, p1);
        if (read2) {
            hpn_sample_rule mate = {};
            mate.mode = HPN_SAMPLE_PICKS, mate.fasta = fasta, mate.picks = kept.data(), mate.n_picks = kept.size();
            Pass p2;
            p2.rule = &mate, p2.out = o2;
            run_pass(ctx, read2, p2);
        }
        for (GzWriter *w : {o1, o2})
            if (w) {
                if (!w->finish()) write_failed();
                t_deflate += w->deflate_seconds(), t_waited += w->waited_seconds(), gz_threads = w->threads();
                delete w;
            }
        fprintf(stderr, "total reads: %lu\npick out: %lu (%lu/%lu=%.6f)\n", (unsigned long)p1.n_records, (unsigned long)p1.n_kept,
                (unsigned long)p1.n_kept, (unsigned long)p1.n_records, (double)p1.n_kept / p1.n_records);
    }
    if (reads_n) {   // get_number_from_file, :227-278
        const std::string mid = std::to_string(reads_n);
        GzWriter *o1 = create_out(out_name(read1, mid.c_str()));
        Pass cnt;
        run_pass(ctx, read1, cnt);
        const unsigned long n = (unsigned long)cnt.n_records;
        fprintf(stderr, "total_reads_num: %ld\n", (long)n);
        fprintf(stderr, "Finished count_read at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
        if (reads_n > n) {
            fprintf(stderr, "pick_count > read_count (%lu > %lu)\n", reads_n, n);
            o1->abandon();
            quick_exit_ok();
        }
        GzWriter *o2 = read2 ? create_out(out_name(read2, mid.c_str())) : nullptr;
        const std::vector<uint64_t> picks = draw_picks(n, reads_n);
        fprintf(stderr, "Start_read at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
        hpn_sample_rule rule = {};
        rule.mode = HPN_SAMPLE_PICKS, rule.fasta = fasta, rule.picks = picks.data(), rule.n_picks = picks.size();
        Pass p1, p2;
        p1.rule = p2.rule = &rule, p1.out = o1, p2.out = o2;
        run_pass(ctx, read1, p1);
        if (read2) run_pass(ctx, read2, p2);
        fprintf(stderr, "End_read at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
        for (GzWriter *w : {o1, o2})
            if (w) {
                if (!w->finish()) write_failed();
                t_deflate += w->deflate_seconds(), t_waited += w->waited_seconds(), gz_threads = w->threads();
                delete w;
            }
        fprintf(stderr, "total reads: %lu\npick out: %lu (%lu/%lu=%.6f)\n", n, reads_n, reads_n, n, (double)reads_n / n);
    }
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] output: deflate %.3f thread-seconds on %d threads, the reading thread waited %.3f s for it\n", t_deflate, gz_threads, t_waited);
    fprintf(stderr, "Finished at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    quick_exit_ok();
}
