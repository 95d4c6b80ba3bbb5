// bam_view -- drop-in for `samtools view` of the samtools-0.1.19 the reference vendors (sam_view.c: main_samview -> process_aln,
// sam.c: samopen / samwrite, bam.c: bam_format1_core) for a BAM input without regions: the records that pass the filters as SAM
// text, as BAM, or counted, byte for byte samtools', with its stderr and status; the filters, the lines' lengths and offsets, the
// SAM text, the BAM output's gather, -Q's rescaled qualities, the BGZF cuts and the CRC-32 of every block made on MI355X through
// libhpngs.
//
//   bam_view [-b | -u | -1] [-h] [-H] [-c] [-x | -X] [-o FILE] [-f INT] [-F INT] [-q INT] [-m INT] [-s FLOAT] [-Q INT]
//            [-l STR] [-r STR] [-R FILE] [-@ INT] <in.bam>
//
// The file is inflated and its records are indexed on the device as bam_sort's are; hpn_bam_view_* classifies every record,
// keeps the records in a store on the device and hands the output back slice by slice.  What the device does not take goes to
// the sequential host route (host/bam_view_host.hpp): float aux fields, an A field of value 0, a NUL inside a name, an unknown
// aux type, a field past its record, -l over a header the reference has words about while it makes its ID -> LB table, -H, a
// damaged or truncated file, stdin, BAM to stdout and a working set beyond the device's memory; HPN_BAM_GPU=0 selects it from the start.  HPN_TIMING=1 says which route ran.  Regions, -S, -t, -T, -L and
// -B are refused with status 2.
#include <sys/stat.h>

#include "../host/bam_view_host.hpp"
#include "../host/bam_tool.hpp"

using namespace hpn;

static const SliceCalls kCalls = {"hpn_bam_view", "bam_view", hpn_bam_view_emit, hpn_bam_view_blocks, hpn_bam_view_payload_dev, hpn_bam_view_stored_dev};

// 0 the output is written, 1 not for the device (the host route starts over; nothing has been said, no output is left), 2 the
// job has ended with the reference's status 1
static int view_device(hpn_ctx *ctx, const view::Options &o, bool timing)
{
    std::string said;
    bamsort::Header hdr;
    if (!open_bam_header(o.in, hdr, said)) return 1;
    // the read-group rule as the session takes it: -R's IDs (and its header, drop_rg's), the IDs whose LB is -l's library
    std::vector<std::string> rg_ids, lib_ids;
    if (o.fn_rg) {
        std::set<std::string> ids;
        if (!view::read_ids(o.fn_rg, ids)) return 1;       // (the host route says what the reference does there)
        rg_ids.assign(ids.begin(), ids.end());
        hdr.text = view::drop_rg(hdr.text, ids);
    }
    if (o.library) {
        std::map<std::string, std::string> tbl;
        if (!rmdup::id_table(hdr.text, tbl)) return 1;     // the reference has words about the header: the host route says them
        for (const auto &kv : tbl)
            if (kv.second == o.library) lib_ids.push_back(kv.first);
    }
    std::vector<const char *> rg_ptr, lib_ptr;
    for (const std::string &id : rg_ids) rg_ptr.push_back(id.c_str());
    for (const std::string &id : lib_ids) lib_ptr.push_back(id.c_str());
    BgzfGpuStream bam;
    BamHeader parsed;
    if (!bam.open(ctx, o.in, parsed)) return 1;
    bam.start();
    const bool text = !o.count && !o.bam_out;
    std::string names;
    std::vector<uint32_t> name_off(1, 0u);
    for (const std::string &n : hdr.name) names += n, name_off.push_back((uint32_t)names.size());
    hpn_view_opts vo;
    memset(&vo, 0, sizeof vo);
    vo.flag_on = (uint32_t)o.flag_on, vo.flag_off = (uint32_t)o.flag_off, vo.min_mapq = o.min_mapq < 0 ? 0u : (uint32_t)o.min_mapq;
    vo.min_qlen = o.min_qlen, vo.qual_scale = o.qual_scale;
    vo.subsample = o.subsample() ? 1u : 0u, vo.seed = o.seed, vo.threshold = o.subsample() ? o.threshold() : 0u;
    vo.emit = o.count ? HPN_VIEW_COUNT : text ? HPN_VIEW_TEXT : HPN_VIEW_BAM;
    vo.flag_style = (uint32_t)o.style;
    vo.n_targets = (int32_t)hdr.name.size(), vo.target_names = names.data(), vo.target_name_off = name_off.data();
    vo.rg_id = o.rg;
    vo.rg_ids = rg_ptr.data(), vo.n_rg_ids = (uint32_t)rg_ptr.size(), vo.has_rg_ids = o.fn_rg ? 1u : 0u;
    vo.lib_ids = lib_ptr.data(), vo.n_lib_ids = (uint32_t)lib_ptr.size(), vo.has_library = o.library ? 1u : 0u;
    int rc = hpn_bam_view_begin(ctx, &vo);
    if (rc == HPN_E_NOMEM) return 1;
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_view_begin");
    FeedRun fed;
    if (!feed_session(ctx, bam, kCalls, hpn_bam_view_add_raw_dev, timing, fed)) return 1;
    hpn_view_result res;
    double t0 = wall_s();
    if (!finish_session(ctx, kCalls, hpn_bam_view_finish, timing, res)) return 1;
    const double t_decide = wall_s() - t0;
    double t_emit = 0, t_copy = 0, t_write = 0;
    uint64_t n_blocks = 0;
    if (o.count) {
        fputs(said.c_str(), stderr);
        printf("%llu\n", (unsigned long long)res.n_out);
        fflush(stdout);
    } else if (text) {
        std::vector<uint8_t> bytes;
        FILE *out = nullptr;
        const bool to_stdout = !o.out || strcmp(o.out, "-") == 0;
        for (uint64_t first = 0;;) {
            hpn_view_text_info ti;
            t0 = wall_s();
            rc = hpn_bam_view_text_emit(ctx, first, kSliceRecords, &ti);
            if (rc == HPN_E_NOMEM && !(out && to_stdout)) {        // the output so far goes; the host route makes it again
                if (out && !to_stdout) fclose(out), unlink(o.out);
                return 1;
            }
            if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_view_text_emit");
            t_emit += wall_s() - t0, t0 = wall_s();
            const uint8_t *d = nullptr;
            uint64_t n = 0;
            if ((rc = hpn_bam_view_text_dev(ctx, &d, &n)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_view_text_dev");
            bytes.resize(n);
            if (n && ((rc = hpn_memcpy_d2h(ctx, bytes.data(), d, n)) != HPN_OK || (rc = hpn_ctx_sync(ctx)) != HPN_OK)) die_hpn(ctx, rc, "hpn_memcpy_d2h");
            t_copy += wall_s() - t0, t0 = wall_s();
            if (!out) {        // behind the first slice: everything the device needs has been allocated by then
                fputs(said.c_str(), stderr);
                out = to_stdout ? stdout : fopen(o.out, "w");
                if (!out) {
                    fprintf(stderr, "[main_samview] fail to open \"%s\" for writing.\n", o.out);
                    return 2;
                }
                if (o.header) {
                    std::string say;
                    const std::string head = view::text_header(hdr, say);
                    fputs(say.c_str(), stderr);
                    fwrite(head.data(), 1, head.size(), out);
                }
            }
            if (fwrite(bytes.data(), 1, (size_t)n, out) != n) {
                fprintf(stderr, "[hpn] bam_view: writing %s failed\n", to_stdout ? "standard output" : o.out);
                leave(2);
            }
            t_write += wall_s() - t0;
            first += ti.n_records;
            if (first >= res.n_out) break;
        }
        if ((to_stdout ? fflush(out) : fclose(out)) != 0) {
            fprintf(stderr, "[hpn] bam_view: writing %s failed\n", to_stdout ? "standard output" : o.out);
            leave(2);
        }
    } else {
        BgzfWriter writer(o.level);
        SliceRun run;
        bool opened = true;
        const int ws = write_session(ctx, kCalls, hdr, res.n_out, o.level, writer, o.out, false, "[hpn] bam_view",
                                     [&](const std::vector<uint8_t> &head_blocks) { return opened = writer.begin(o.out, head_blocks); }, run);
        if (ws == kSlicesNoOutput && !opened) {
            fputs(said.c_str(), stderr);
            fprintf(stderr, "[main_samview] fail to open \"%s\" for writing.\n", o.out);
            return 2;
        }
        if (ws != kSlicesDone) return 1;
        fputs(said.c_str(), stderr);
        t_emit = run.t_emit, t_copy = run.t_copy, t_write = run.t_hand, n_blocks = run.n_blocks;
    }
    if (timing)
        fprintf(stderr, "[hpn] bam_view: inflate + record index %.3f s, classify + store %.3f s, scans + order %.3f s, %s %.3f s, copies to the host %.3f s, "
                        "%s %.3f s; %llu batches, %llu records in, %llu kept, %llu text bytes, %llu blocks\n",
                fed.t_ingest, fed.t_store, t_decide, text ? "format" : "gather + scale + cuts + crc", t_emit, t_copy, text ? "fwrite" : "handing to the writer",
                t_write, (unsigned long long)fed.n_batches, (unsigned long long)res.n_records, (unsigned long long)res.n_out, (unsigned long long)res.text_bytes,
                (unsigned long long)n_blocks);
    return 0;
}

int main(int argc, char *argv[])
{
    view::Options o;
    return run_tool(
        "bam_view",
        [&]() { return view::parse_args(argc, argv, o); },
        [&]() {
            const bool bam_to_stdout = o.bam_out && !o.count && (!o.out || strcmp(o.out, "-") == 0);
            return bam_gpu_enabled() && !o.header_only && !bam_to_stdout && strcmp(o.in, "-") != 0 && access(o.in, R_OK) == 0;
        },
        [&](hpn_ctx *ctx, bool timing) { return view_device(ctx, o, timing); },
        [&]() { return view::view_on_host(o); });
}
