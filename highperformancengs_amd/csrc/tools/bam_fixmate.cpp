// bam_fixmate -- drop-in for `samtools fixmate` of the samtools-0.1.19 the reference vendors (bam_mate.c: bam_mating ->
// bam_mating_core): a name-grouped BAM with every record's mate refID, mate pos, insert size and mate flag bits filled in and
// the CT:Z field of bam_template_cigar appended, byte for byte samtools', with its status; the pairing, the output's order, the
// rewritten records, the BGZF cuts and the CRC-32 of every block made on MI355X through libhpngs.
//
//   bam_fixmate [-r] <in.nameSrt.bam> <out.nameSrt.bam>
//
// The file is inflated and its records are indexed on the device as bam_sort's are; hpn_bam_fixmate_* classifies every record,
// keeps the records in a store on the device and hands the output back slice by slice.  A CIGAR op above 8, a name with a NUL
// inside, a refID beyond the header, a damaged or truncated file, stdin or stdout and a working set beyond the device's memory go
// to the sequential host route (host/bam_fixmate_host.hpp); HPN_BAM_GPU=0 selects it from the start.  HPN_TIMING=1 says which
// route ran.
#include <sys/stat.h>

#include "../host/bam_fixmate_host.hpp"
#include "../host/bam_tool.hpp"

using namespace hpn;

static const SliceCalls kCalls = {"hpn_bam_fixmate", "bam_fixmate", hpn_bam_fixmate_emit, hpn_bam_fixmate_blocks, hpn_bam_fixmate_payload_dev, hpn_bam_fixmate_stored_dev};

// 0 the output is written, 1 not for the device (the host route starts over; nothing has been said, no output is left)
static int fixmate_device(hpn_ctx *ctx, const fixmate::Options &o, bool timing)
{
    std::string said;
    bamsort::Header hdr;
    if (!open_bam_header(o.in, hdr, said)) return 1;   // on the host: its blocks are the writer's first, its lengths the device's table
    BgzfGpuStream bam;
    BamHeader parsed;
    if (!bam.open(ctx, o.in, parsed)) return 1;
    bam.start();
    int rc = hpn_bam_fixmate_begin(ctx, o.remove_reads ? 1 : 0, (int32_t)hdr.len.size(), (const uint32_t *)hdr.len.data());
    if (rc == HPN_E_NOMEM) return 1;
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_fixmate_begin");
    FeedRun fed;
    if (!feed_session(ctx, bam, kCalls, hpn_bam_fixmate_add_raw_dev, timing, fed)) return 1;
    hpn_fixmate_result res;
    const double t0 = wall_s();
    if (!finish_session(ctx, kCalls, hpn_bam_fixmate_finish, timing, res)) return 1;
    const double t_decide = wall_s() - t0;
    BgzfWriter writer(-1);
    SliceRun run;
    // (the output is a file: whenever the device's memory runs out it can go, and the host route makes it again, or says why it cannot)
    const int ws = write_session(ctx, kCalls, hdr, res.n_out, -1, writer, o.out, false, "[hpn] bam_fixmate",
                                 [&](const std::vector<uint8_t> &head_blocks) { return writer.begin(o.out, head_blocks); }, run);
    if (ws != kSlicesDone) return 1;
    fputs(said.c_str(), stderr);
    if (timing)
        fprintf(stderr, "[hpn] bam_fixmate: inflate + record index %.3f s, classify + store %.3f s, names + roles + order + patches %.3f s, "
                        "gather + patch + cuts + crc %.3f s, copies to the host %.3f s, handing to the writer %.3f s; %llu batches, %llu records in, %llu out, "
                        "%llu pairs, %llu singletons, %llu CT fields (%llu bytes), %llu blocks; writer: %.3f s deflating (all threads), %.3f s waited for\n",
                fed.t_ingest, fed.t_store, t_decide, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)fed.n_batches, (unsigned long long)res.n_records,
                (unsigned long long)res.n_out, (unsigned long long)res.n_pairs, (unsigned long long)res.n_singletons, (unsigned long long)res.n_tags,
                (unsigned long long)res.bytes_added, (unsigned long long)run.n_blocks, writer.deflate_seconds(), writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    fixmate::Options o;
    return run_tool(
        "bam_fixmate",
        [&]() { return fixmate::parse_args(argc, argv, o) ? 0 : 1; },
        [&]() {
            return bam_gpu_enabled() && strcmp(o.in, "-") != 0 && strcmp(o.out, "-") != 0 && access(o.in, R_OK) == 0;
        },
        [&](hpn_ctx *ctx, bool timing) { return fixmate_device(ctx, o, timing); },
        [&]() { return fixmate::fixmate_on_host(o); });
}
