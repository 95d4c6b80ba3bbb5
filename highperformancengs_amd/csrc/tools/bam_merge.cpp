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

static const SliceCalls kCalls = {"hpn_bam_merge", "bam_merge", hpn_bam_merge_emit, hpn_bam_merge_blocks, hpn_bam_merge_payload_dev, hpn_bam_merge_stored_dev};

// 0 the output is written, 1 not for the device (the host route starts over; nothing has been said, no output is left), 2 the
// output could not be created: the reference's status 1
// hdr, said: what bammerge::prepare made of the inputs' headers and what the reference would have remarked on the way
static int merge_device(hpn_ctx *ctx, const bammerge::Options &o, const bamsort::Header &hdr, const std::string &said, bool timing)
{
    int rc = hpn_bam_merge_begin(ctx);
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_merge_begin");
    FeedRun fed;
    for (const char *path : o.in) {
        BgzfGpuStream bam;      // one stream per input, one after the other
        BamHeader parsed;
        if (!bam.open(ctx, path, parsed)) return 1;
        bam.start();
        if ((rc = hpn_bam_merge_next_file(ctx)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_merge_next_file");
        if (!feed_session(ctx, bam, kCalls, hpn_bam_merge_add_raw_dev, timing, fed)) return 1;
    }
    hpn_bammerge_result res;
    const double t0 = wall_s();
    if (!finish_session(ctx, kCalls, hpn_bam_merge_finish, timing, res)) return 1;
    const double t_sort = wall_s() - t0;
    const int level = bammerge::level_of(o);
    const std::string path = bammerge::output_path(o);
    BgzfWriter writer(level);
    SliceRun run;
    const int ws = write_session(ctx, kCalls, hdr, res.n_records, level, writer, path.c_str(), strcmp(o.out, "-") == 0, "bam_merge",
                                 [&](const std::vector<uint8_t> &head_blocks) {
        fputs(said.c_str(), stderr);
        if (writer.begin(path.c_str(), head_blocks)) return true;
        fputs("[bam_merge_core2] fail to create the output file.\n", stderr);
        return false;
    }, run);
    if (ws == kSlicesNoMem) return 1;
    if (ws == kSlicesNoOutput) return 2;
    if (timing)
        fprintf(stderr, "[hpn] bam_merge: inflate + record index %.3f s, keys + store %.3f s, running maximum + sort + offsets %.3f s, gather + cuts + crc %.3f s, "
                        "copies to the host %.3f s, handing to the writer %.3f s; %llu files, %llu batches, %llu records, %llu lifted, %u key bits, %llu blocks; "
                        "writer: %.3f s deflating (all threads), %.3f s waited for\n",
                fed.t_ingest, fed.t_store, t_sort, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)res.n_files, (unsigned long long)fed.n_batches,
                (unsigned long long)res.n_records, (unsigned long long)res.n_lifted, res.sort_bits, (unsigned long long)run.n_blocks, writer.deflate_seconds(),
                writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    bammerge::Options o;
    std::string said;
    bamsort::Header hdr;
    return run_tool(
        "bam_merge",
        [&]() { return bammerge::parse_args(argc, argv, o); },
        [&]() {
            bool device = bam_gpu_enabled() && !o.by_name && !o.rg;
            for (const char *p : o.in) device = device && strcmp(p, "-") != 0;
            // on the host: the header rule (a job it ends goes to the host route, which says why), and the header's blocks are the writer's first
            return device && bammerge::prepare(o, hdr, said) == 0;
        },
        [&](hpn_ctx *ctx, bool timing) { return merge_device(ctx, o, hdr, said, timing); },
        [&]() { return bammerge::merge_on_host(o); });
}
