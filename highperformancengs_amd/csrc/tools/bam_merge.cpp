// bam_merge -- drop-in for `samtools merge` of the samtools-0.1.19 the reference vendors (bam_sort.c: bam_merge ->
// bam_merge_core2): several BAMs -- sorted or not, the reference never checks -- merged into the one file every BAM tool here asks
// for, byte for byte samtools', with the keys, the running maximum inside every input, the sort, the gather into merged order,
// the BGZF cuts and the CRC-32 of every block made on MI355X through libhpngs.
//
//   bam_merge [-nr] [-h inh.sam] [-u1f] [-l INT] [-@ INT] <out.bam> <in1.bam> <in2.bam> [...]
//
// Messages and status are the reference's: 1 for fewer than three file arguments, an output that exists without -f, an input
// or -h file that cannot be opened, target names that differ, a -h file whose @SQ lines do not fit; 0 else.  -R is not supported
// (status 2, nothing is opened).  Every input is inflated and its records are indexed on the device, one input after the other,
// into one hpn_bam_merge_* session, which keeps the records in a store on the device and hands the merged output back slice by
// slice.  -n, -r, a record with the heap's HEAP_EMPTY key, a damaged or truncated input, an empty BGZF block in mid-file and a
// working set beyond the device's memory go to the sequential host route (host/bam_merge_host.hpp); HPN_BAM_GPU=0 selects it
// from the start.  HPN_TIMING=1 says which route ran.
#include <sys/stat.h>

#include "../host/bam_merge_host.hpp"
#include "../host/bam_tool.hpp"

using namespace hpn;

// 0 the output is written, 1 not for the device (the host route starts over; nothing has been said, no output is left)
// hdr, said: what bammerge::prepare made of the inputs' headers and what the reference would have remarked on the way
static int merge_device(hpn_ctx *ctx, const bammerge::Options &o, const bamsort::Header &hdr, const std::string &said, bool timing)
{
    int rc = hpn_bam_merge_begin(ctx);
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_merge_begin");
    double t_ingest = 0, t_store = 0, t_sort = 0, t0;
    uint64_t n_batches = 0;
    for (const char *path : o.in) {
        BgzfGpuStream bam;      // one stream per input, one after the other
        BamHeader parsed;
        if (!bam.open(ctx, path, parsed)) return 1;
        bam.start();
        if ((rc = hpn_bam_merge_next_file(ctx)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_merge_next_file");
        const bool fed = each_batch(bam, &t_ingest, [&](const BgzfDevice &) {
            hpn_bammerge_info mi;
            t0 = wall_s();
            rc = hpn_bam_merge_add_raw_dev(ctx, bam.d_raw(), &mi);
            if (rc == HPN_E_NOMEM) return false;               // the working set does not fit the device
            if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_merge_add_raw_dev");
            t_store += wall_s() - t0, ++n_batches;
            if (mi.bad_record >= 0) {
                if (timing)
                    fprintf(stderr, "[hpn] bam_merge: record %lld (refID %d, pos %d) is outside the device's domain (reason %u)\n", (long long)mi.bad_record,
                            mi.bad_tid, mi.bad_pos, mi.reason);
                return false;
            }
            return true;
        });
        if (!fed) return 1;
    }
    hpn_bammerge_result res;
    t0 = wall_s();
    rc = hpn_bam_merge_finish(ctx, &res);
    if (rc == HPN_E_NOMEM) return 1;
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_merge_finish");
    if (res.bad_record >= 0) return 1;
    t_sort = wall_s() - t0;
    const int level = bammerge::level_of(o);
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), level, head_blocks)) return 1;
    const std::string path = bammerge::output_path(o);
    const bool to_stdout = strcmp(o.out, "-") == 0;
    BgzfWriter writer(level);
    SliceRun run;
    bool refused = false;
    const SliceCalls calls = {"hpn_bam_merge", hpn_bam_merge_emit, hpn_bam_merge_blocks, hpn_bam_merge_payload_dev, hpn_bam_merge_stored_dev};
    // (what has gone to stdout cannot be taken back: behind the first slice the device's memory running out is an error there)
    const int ws = write_slices(ctx, calls, res.n_records, level, writer, to_stdout, [&]() {
        fputs(said.c_str(), stderr);
        if (!writer.begin(path.c_str(), head_blocks)) {
            fputs("[bam_merge_core2] fail to create the output file.\n", stderr);
            refused = true;
            return false;
        }
        return true;
    }, run);
    if (ws == kSlicesNoOutput) return refused ? 2 : 0;
    if (ws == kSlicesNoMem) {   // the output so far goes; the host route makes it again
        if (run.created) writer.abandon();
        if (run.created && !to_stdout) unlink(path.c_str());
        return 1;
    }
    if (!writer.finish()) {
        fprintf(stderr, "bam_merge: writing %s failed\n", path.c_str());
        leave(2);
    }
    if (timing)
        fprintf(stderr, "[hpn] bam_merge: inflate + record index %.3f s, keys + store %.3f s, running maximum + sort + offsets %.3f s, gather + cuts + crc %.3f s, "
                        "copies to the host %.3f s, handing to the writer %.3f s; %llu files, %llu batches, %llu records, %llu lifted, %u key bits, %llu blocks; "
                        "writer: %.3f s deflating (all threads), %.3f s waited for\n",
                t_ingest, t_store, t_sort, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)res.n_files, (unsigned long long)n_batches,
                (unsigned long long)res.n_records, (unsigned long long)res.n_lifted, res.sort_bits, (unsigned long long)run.n_blocks, writer.deflate_seconds(),
                writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    stamp("main");
    bammerge::Options o;
    const int early = bammerge::parse_args(argc, argv, o);
    if (early) return early;
    const bool timing = getenv("HPN_TIMING") != nullptr;
    bool device = bam_gpu_enabled() && !o.by_name && !o.rg;
    for (const char *p : o.in) device = device && strcmp(p, "-") != 0;
    std::string said;
    bamsort::Header hdr;
    // on the host: the header rule (a job it ends goes to the host route, which says why), and the header's blocks are the writer's first
    if (device && bammerge::prepare(o, hdr, said) == 0) {
        hpn_ctx *ctx = open_tool_ctx();
        stamp("context created");
        const int r = merge_device(ctx, o, hdr, said, timing);
        if (timing) fprintf(stderr, "[hpn] bam_merge: %s\n", r != 1 ? "device route" : "device route abandoned: host route");
        if (r == 0) {
            stamp("finished");
            quick_exit_ok();
        }
        if (r == 2) leave(1);      // the output could not be created: the reference's status
    } else if (timing) {
        fprintf(stderr, "[hpn] bam_merge: host route\n");
    }
    const int status = bammerge::merge_on_host(o);
    stamp("finished");
    leave(status);
}
