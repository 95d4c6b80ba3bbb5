// bamSplitChr -- drop-in for the reference tool of the same name (bamSplitChr.c): one BAM per @SQ target, each with the
// input's header, from an indexed coordinate-sorted BAM; the target boundaries, the domain checks, the BGZF cuts, the CRC-32
// of every block and (uncompressed output) the blocks themselves made on MI355X through libhpngs.
//
//   bamSplitChr [-o PREFIX] [-1 x] [-u x] [-h] a.bam b.bam ...
//
// Writes PREFIX_<target>.bam per target (bamSplitChr.c:130); without -o the prefix is the input's path, and -o holds for the
// first input only (:141).  The option string is the reference's, "o:w:r:s:u:1:h?" (:88): -u and -1 TAKE AN ARGUMENT.
// Like the reference it insists on <bam>.bai (:128) although it reads the file front to back: for a coordinate-sorted file
// with a matching index bam_fetch(tid, 0, 1 << 29) per target visits exactly the target's records, in file order.  Where
// that does not hold -- records out of order, a placed record without a position, pos >= 2^29, an index of another file --
// the reference's outputs depend on the index's chunk lists; the tool says which record or what of the index, removes the
// input's outputs and exits with status 2.
#include <err.h>
#include <getopt.h>
#include <sys/stat.h>
#include <zlib.h>

#include "../host/bam_gpu.hpp"
#include "../host/bgzf_writer.hpp"
#include "../host/report.hpp"

using namespace hpn;

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s [-o OUTFILE_PREFIX] [-1 x] [-u x] [-h] bamFile1 bamFile2 ..\n"
            "  Splits indexed, coordinate-sorted BAM files into one BAM per target: PREFIX_<target>.bam\n"
            "  (MI355X build of HighPerformanceNGS bamSplitChr).\n\n"
            "   [-o PREFIX]   output prefix (first input only; default: the input's path)\n"
            "   -1 x          fast compression (the option takes an argument, as in the reference)\n"
            "   -u x          uncompressed output (likewise)\n"
            "   [-h]          this help\n\n",
            prog);
    exit(1);
}

// The file's BGZF blocks one after the other on the host (zlib): the header for both routes, the records for the host route.
struct HostBgzf {
    FILE *f = nullptr;
    std::vector<uint8_t> buf, raw;
    size_t at = 0;
    bool bad = false;
    ~HostBgzf() { if (f) fclose(f); }
    bool open(const char *path) { return (f = fopen(path, "rb")) != nullptr; }
    bool next_block()
    {
        uint8_t h[18];
        const size_t got = fread(h, 1, 18, f);
        if (got == 0) return false;
        if (got != 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4) || h[12] != 'B' || h[13] != 'C') return bad = true, false;
        const uint32_t bsize = (h[16] | (h[17] << 8)) + 1u, xlen = h[10] | (h[11] << 8);
        if (bsize < xlen + 20u || xlen < 6u) return bad = true, false;
        raw.resize(bsize - 18);
        if (fread(raw.data(), 1, raw.size(), f) != raw.size()) return bad = true, false;
        uint32_t isize;
        memcpy(&isize, raw.data() + raw.size() - 4, 4);
        if (isize > 65536u) return bad = true, false;
        buf.resize(isize), at = 0;
        if (!isize) return true;
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return bad = true, false;
        zs.next_in = raw.data() + (xlen - 6), zs.avail_in = (uInt)(raw.size() - (xlen - 6) - 8);
        zs.next_out = buf.data(), zs.avail_out = isize;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        if (rc != Z_STREAM_END || zs.avail_out != 0) return bad = true, false;
        return true;
    }
    bool read(void *dst, size_t n)       // false: the stream ends (or fails) before n bytes
    {
        uint8_t *d = (uint8_t *)dst;
        while (n) {
            if (at == buf.size() && !next_block()) return false;
            const size_t k = buf.size() - at < n ? buf.size() - at : n;
            memcpy(d, buf.data() + at, k);
            d += k, at += k, n -= k;
        }
        return true;
    }
};

struct Header {
    std::vector<uint8_t> bytes;            // magic .. the last target's length, verbatim
    std::vector<std::string> name;
    std::vector<int32_t> len;
};

static bool read_header(HostBgzf &in, Header &h)
{
    auto take = [&](size_t n) {
        const size_t o = h.bytes.size();
        h.bytes.resize(o + n);
        return in.read(h.bytes.data() + o, n);
    };
    auto i32 = [&](size_t o) { int32_t v; memcpy(&v, h.bytes.data() + o, 4); return v; };
    if (!take(8) || memcmp(h.bytes.data(), "BAM\1", 4)) return false;
    const int32_t l_text = i32(4);
    if (l_text < 0 || !take((size_t)l_text + 4)) return false;
    const int32_t n_ref = i32(8 + (size_t)l_text);
    if (n_ref < 0) return false;
    for (int32_t t = 0; t < n_ref; ++t) {
        size_t o = h.bytes.size();
        if (!take(4)) return false;
        const int32_t l_name = i32(o);
        if (l_name < 1 || !take((size_t)l_name + 4)) return false;
        h.name.emplace_back((const char *)h.bytes.data() + o + 4, strnlen((const char *)h.bytes.data() + o + 4, (size_t)l_name));
        h.len.push_back(i32(o + 4 + (size_t)l_name));
    }
    return true;
}

// samopen failed (bamSplitChr.c:125-127).  A file that cannot be opened: libbam's knet_open has said "open: <why>" by then and
// what err() appends is "Invalid argument" (recorded: tests/golden/split/manifest.json, missing_input).
[[noreturn]] static void fail_open(const char *path, bool unopened)
{
    if (unopened) {
        fprintf(stderr, "open: %s\n", strerror(errno));
        errno = EINVAL;
    }
    fflush(NULL);
    err(1, "bam2bed: Fail to open BAM file %s\n", path);
}

// <bam>.bai, or x.bai for x.bam (bam_index.c: bam_index_load_local)
static std::string index_path(const char *bam)
{
    std::string a = std::string(bam) + ".bai", b = bam;
    if (access(a.c_str(), R_OK) == 0) return a;
    if (b.size() > 3 && b.compare(b.size() - 3, 3, "bam") == 0) {
        b.replace(b.size() - 3, 3, "bai");
        if (access(b.c_str(), R_OK) == 0) return b;
    }
    return "";
}

// What of the index the domain asks for: magic, n_ref, and per target the record count of samtools' pseudo-bin 37450
// (n_mapped + n_unmapped; -1 where the index carries none).  "" or what is wrong with it.
static std::string read_index(const std::string &path, int32_t n_ref, std::vector<int64_t> &pseudo)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return "cannot be read";
    std::string why;
    auto get = [&](void *p, size_t n) { return fread(p, 1, n, f) == n; };
    char magic[4];
    int32_t n = 0;
    if (!get(magic, 4) || memcmp(magic, "BAI\1", 4)) why = "is no BAM index (magic)";
    else if (!get(&n, 4)) why = "is truncated";
    else if (n != n_ref) why = "has " + std::to_string(n) + " targets, the header " + std::to_string(n_ref);
    pseudo.assign((size_t)(n_ref > 0 ? n_ref : 0), -1);
    for (int32_t t = 0; why.empty() && t < n; ++t) {
        int32_t n_bin = 0, n_intv = 0;
        if (!get(&n_bin, 4) || n_bin < 0) { why = "is truncated"; break; }
        for (int32_t b = 0; b < n_bin; ++b) {
            uint32_t bin;
            int32_t n_chunk;
            if (!get(&bin, 4) || !get(&n_chunk, 4) || n_chunk < 0) { why = "is truncated"; break; }
            std::vector<uint64_t> ch((size_t)n_chunk * 2);
            if (n_chunk && !get(ch.data(), ch.size() * 8)) { why = "is truncated"; break; }
            if (bin == 37450u && n_chunk == 2) pseudo[(size_t)t] = (int64_t)(ch[2] + ch[3]);
        }
        if (!why.empty()) break;
        if (!get(&n_intv, 4) || n_intv < 0) { why = "is truncated"; break; }
        std::vector<uint64_t> lin((size_t)n_intv);             // (read, not skipped: a seek succeeds past the end of a cut-off file)
        if (n_intv && !get(lin.data(), lin.size() * 8)) why = "is truncated";
    }
    fclose(f);
    return why;
}

// The outputs of one input: target after target, one file open at a time.
struct Sink {
    BgzfWriter *w;
    const Header *hdr;
    std::string prefix;
    const std::vector<uint8_t> *head_blocks;
    int32_t cur = 0;                  // the target whose file is open or comes next
    bool is_open = false;
    std::vector<std::string> made;
    std::string path(int32_t t) const { return prefix + "_" + hdr->name[(size_t)t] + ".bam"; }
    void open_cur()
    {
        if (is_open) return;
        const std::string p = path(cur);
        if (!w->begin(p.c_str(), *head_blocks)) {
            fflush(NULL);
            err(1, "[main_samview] fail to open \"%s\" for writing.\n", p.c_str());
        }
        made.push_back(p);
        is_open = true;
    }
    void close_cur()
    {
        open_cur();                   // (a target without records: header + the empty last block)
        if (!w->finish()) {
            fprintf(stderr, "bamSplitChr: writing %s failed\n", path(cur).c_str());
            is_open = false;
            remove_all();
            leave(2);
        }
        is_open = false, ++cur;
    }
    void move_to(int32_t t) { while (cur < t) close_cur(); open_cur(); }
    void block(int32_t t, const uint8_t *p, uint32_t n, uint32_t crc, bool have_crc)
    {
        move_to(t);
        w->add(p, n, crc, have_crc);
    }
    void framed(int32_t t, const uint8_t *p, size_t n)
    {
        move_to(t);
        w->add_framed(p, n);
    }
    void finish_all() { while (cur < (int32_t)hdr->name.size()) close_cur(); }
    void remove_all()
    {
        if (is_open) w->abandon();
        is_open = false;
        for (const std::string &p : made) unlink(p.c_str());
        made.clear();
    }
};

static const char *const kReasons[] = {"", "refID outside the header's targets", "pos outside [0, 2^29)", "refID goes backwards", "pos goes backwards"};

struct Refusal {
    bool set = false;
    long long ordinal = 0;
    int32_t tid = 0, pos = 0;
    uint32_t reason = 0;
};

// 0 done, 1 not decodable on the device (the host route starts over), 2 refused
static int split_device(hpn_ctx *ctx, const char *path, Sink &sink, int32_t n_ref, int level, std::vector<uint64_t> &counts, Refusal &bad)
{
    BgzfGpuStream bam;
    BamHeader parsed;
    if (!bam.open(ctx, path, parsed) || parsed.n_targets() != n_ref) return 1;
    bam.start();
    int rc = hpn_bam_split_begin(ctx, n_ref, level == 0);
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_split_begin");
    std::vector<hpn_split_block> blocks;
    std::vector<uint8_t> bytes;
    double t_ingest = 0, t_split = 0, t_copy = 0, t_hand = 0, t0;     // HPN_TIMING: where the main thread's time goes
    uint64_t n_batches = 0, n_blocks = 0, n_bytes = 0;
    auto take = [&](const hpn_split_info &si) {
        if (!si.n_blocks) return;
        uint64_t nb = 0;
        t0 = wall_s();
        blocks.resize(si.n_blocks);
        if ((rc = hpn_bam_split_blocks(ctx, 0, blocks.data(), blocks.size(), &nb)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_split_blocks");
        const uint8_t *d = nullptr;
        uint64_t n = 0;
        rc = level == 0 ? hpn_bam_split_stored_dev(ctx, &d, &n) : hpn_bam_split_payload_dev(ctx, &d, &n);
        if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_split_payload_dev");
        bytes.resize(n);
        if (n && ((rc = hpn_memcpy_d2h(ctx, bytes.data(), d, n)) != HPN_OK || (rc = hpn_ctx_sync(ctx)) != HPN_OK)) die_hpn(ctx, rc, "hpn_memcpy_d2h");
        t_copy += wall_s() - t0, t0 = wall_s();
        n_blocks += si.n_blocks, n_bytes += n;
        stamp("split: blocks and bytes of a batch on the host");
        if (level == 0) {             // the image holds the blocks one after the other: a target's run is one append
            uint64_t at = 0;
            for (size_t k = 0; k < nb;) {
                size_t e = k;
                uint64_t len = 0;
                while (e < nb && blocks[e].tid == blocks[k].tid) len += (uint64_t)blocks[e].len + 31, ++e;
                sink.framed(blocks[k].tid, bytes.data() + at, len);
                at += len, k = e;
            }
        } else {
            for (size_t k = 0; k < nb; ++k) sink.block(blocks[k].tid, bytes.data() + blocks[k].off, blocks[k].len, blocks[k].crc, true);
        }
        t_hand += wall_s() - t0;
    };
    for (;;) {
        hpn_raw_info info;
        t0 = wall_s();
        const int r = bam.next(&info);
        t_ingest += wall_s() - t0;
        if (r < 0) return 1;
        if (r == 0) break;
        if (!info.n_records) continue;
        hpn_split_info si;
        t0 = wall_s();
        if ((rc = hpn_bam_split_add_raw_dev(ctx, bam.d_raw(), 0, &si)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_split_add_raw_dev");
        t_split += wall_s() - t0, ++n_batches;
        if (si.bad_record >= 0) {
            bad.set = true, bad.ordinal = si.bad_record, bad.tid = si.bad_tid, bad.pos = si.bad_pos, bad.reason = si.reason;
            return 2;
        }
        take(si);
    }
    hpn_split_info si;
    if ((rc = hpn_bam_split_add_raw_dev(ctx, nullptr, 1, &si)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_split_add_raw_dev");
    take(si);
    hpn_split_result res;
    counts.assign((size_t)n_ref, 0);
    if ((rc = hpn_bam_split_finish(ctx, &res, counts.data())) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_split_finish");
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] split: inflate + index %.3f s, keys + cuts + crc + framing %.3f s, copies to the host %.3f s, handing to the writer %.3f s; "
                        "%llu batches, %llu blocks, %llu bytes copied\n",
                t_ingest, t_split, t_copy, t_hand, (unsigned long long)n_batches, (unsigned long long)n_blocks, (unsigned long long)n_bytes);
    return 0;
}

// The same on the host: the same rules, the same cuts, the CRC-32 by the writer's threads.  0 done, 2 refused
static int split_host(HostBgzf &in, Sink &sink, int32_t n_ref, std::vector<uint64_t> &counts, Refusal &bad)
{
    counts.assign((size_t)n_ref, 0);
    int32_t open_tid = -1;
    auto emit = [&](const uint8_t *p, uint32_t n) { sink.block(open_tid, p, n, 0, false); };
    BgzfCutter<decltype(emit)> cut(emit);
    std::vector<uint8_t> rec;
    bool have = false;
    int32_t ptid = 0, ppos = 0;
    for (long long ord = 0;; ++ord) {
        int32_t bs;
        if (!in.read(&bs, 4)) break;
        if (bs < 32) break;                                 // (bam_read1 gives up here; so does the fetch)
        rec.resize((size_t)bs + 4);
        memcpy(rec.data(), &bs, 4);
        if (!in.read(rec.data() + 4, (size_t)bs)) break;
        int32_t tid, pos;
        memcpy(&tid, rec.data() + 4, 4), memcpy(&pos, rec.data() + 8, 4);
        uint32_t reason = 0;
        if (tid < -1 || tid >= n_ref) reason = 1;
        else if (tid >= 0 && (pos < 0 || pos >= (1 << 29))) reason = 2;
        else if (have && (uint32_t)tid < (uint32_t)ptid) reason = 3;
        else if (have && tid == ptid && tid >= 0 && pos < ppos) reason = 4;
        if (reason) {
            bad.set = true, bad.ordinal = ord, bad.tid = tid, bad.pos = pos, bad.reason = reason;
            return 2;
        }
        if (tid != open_tid) cut.close(), open_tid = tid;
        have = true, ptid = tid, ppos = pos;
        if (tid < 0) continue;
        ++counts[(size_t)tid];
        cut.record(rec.data(), rec.size());
    }
    cut.close();
    return 0;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *outfile = nullptr;
    int level = -1;
    stamp("main");
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "o:w:r:s:u:1:h?")) != -1) {
        switch (opt) {
        case 'o': outfile = optarg; break;
        case 'u': level = 0; break;
        case '1': level = 1; break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    char **infiles = argv + optind;
    const int n_in = argc - optind;
    const long long begin = usec();
    const bool timing = getenv("HPN_TIMING") != nullptr;
    if (timing) fprintf(stderr, "[hpn] zlib %s\n", zlibVersion());

    hpn_ctx *ctx = nullptr;
    BgzfWriter writer(level);
    for (int i = 0; i < n_in; ++i) {
        if (!outfile) outfile = infiles[i];
        Header hdr;
        {
            HostBgzf in;
            if (!in.open(infiles[i])) fail_open(infiles[i], true);
            if (!read_header(in, hdr)) fail_open(infiles[i], false);
        }
        const int32_t n_ref = (int32_t)hdr.name.size();
        const std::string bai = index_path(infiles[i]);
        if (bai.empty()) {
            fprintf(stderr, "[bam_index_load] fail to load BAM index.\n");
            fprintf(stderr, "bam2bed: BAM indexing file is not available.\n");
            leave(1);
        }
        std::vector<int64_t> pseudo;
        const std::string wrong = read_index(bai, n_ref, pseudo);
        if (!wrong.empty()) {
            fprintf(stderr, "bamSplitChr: %s: the index %s: outside the tool's domain\n", infiles[i], wrong.c_str());
            leave(2);
        }
        for (int32_t t = 0; t < n_ref; ++t)
            if (strlen(outfile) + 1 + hdr.name[(size_t)t].size() + 4 >= 256) {      // sprintf into fn_out[256] (bamSplitChr.c:116,130)
                fprintf(stderr, "bamSplitChr: %s: the output name of target %d does not fit the reference's 256 bytes: outside the tool's domain\n", infiles[i], t);
                leave(2);
            }
        std::vector<uint8_t> head_blocks;
        if (!bgzf_plain_blocks(hdr.bytes.data(), hdr.bytes.size(), level, head_blocks)) {
            fprintf(stderr, "bamSplitChr: deflating the header failed\n");
            leave(2);
        }
        std::vector<uint64_t> counts;
        Refusal bad;
        Sink sink{&writer, &hdr, outfile, &head_blocks};
        int r = 1;
        if (bam_gpu_enabled() && n_ref > 0) {
            if (!ctx) {
                ctx = open_tool_ctx();
                stamp("context created");
            }
            r = split_device(ctx, infiles[i], sink, n_ref, level, counts, bad);
            if (r == 1) sink.remove_all(), sink = Sink{&writer, &hdr, outfile, &head_blocks};
            if (timing) fprintf(stderr, "[hpn] GPU split%s\n", r == 1 ? "  (abandoned: not decodable on the GPU)" : "");
        }
        if (r == 1 && n_ref > 0) {
            HostBgzf in;
            Header again;
            if (!in.open(infiles[i]) || !read_header(in, again)) fail_open(infiles[i], false);
            r = split_host(in, sink, n_ref, counts, bad);
        } else if (r == 1) {
            r = 0;                                            // no target: no output
        }
        if (r == 0) {
            sink.finish_all();
            for (int32_t t = 0; t < n_ref; ++t)
                if (pseudo[(size_t)t] >= 0 && (uint64_t)pseudo[(size_t)t] != counts[(size_t)t]) {
                    sink.remove_all();
                    fprintf(stderr, "bamSplitChr: %s: the index counts %lld records of target %d, the file holds %llu: outside the tool's domain\n", infiles[i],
                            (long long)pseudo[(size_t)t], t, (unsigned long long)counts[(size_t)t]);
                    leave(2);
                }
        } else {
            sink.remove_all();
            fprintf(stderr, "bamSplitChr: %s: record %lld (refID %d, pos %d): %s: outside the tool's domain\n", infiles[i], bad.ordinal, bad.tid, bad.pos,
                    kReasons[bad.reason < 5 ? bad.reason : 0]);
            leave(2);
        }
        stamp("outputs written");
        for (int32_t t = 0; t < n_ref; ++t)
            fprintf(stderr, "chr: %s\tchr_len: %d\treads_count: %u at %.3f s\n", hdr.name[(size_t)t].c_str(), hdr.len[(size_t)t], (uint32_t)counts[(size_t)t],
                    (double)(usec() - begin) / CLOCKS_PER_SEC);
        if (timing)
            fprintf(stderr, "[hpn] writer: %.3f s deflating (all threads), %.3f s the main thread waited for it\n", writer.deflate_seconds(), writer.waited_seconds());
        outfile = nullptr;
        fprintf(stderr, "splited %s into each chromosome at %.3f s\n", infiles[i], (double)(usec() - begin) / CLOCKS_PER_SEC);
    }
    stamp("finished");
    quick_exit_ok();
}
