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
    double t_ingest = 0, t_store = 0, t_decide = 0, t0;
    uint64_t n_batches = 0;
    auto outside = [&](long long rec, int tid, int pos, unsigned reason) {
        if (timing) fprintf(stderr, "[hpn] bam_fixmate: record %lld (refID %d, pos %d) is outside the device's domain (reason %u)\n", rec, tid, pos, reason);
        return 1;
    };
    const bool fed = each_batch(bam, &t_ingest, [&](const BgzfDevice &) {
        hpn_fixmate_info fi;
        t0 = wall_s();
        rc = hpn_bam_fixmate_add_raw_dev(ctx, bam.d_raw(), &fi);
        if (rc == HPN_E_NOMEM) return false;               // the working set does not fit the device
        if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_fixmate_add_raw_dev");
        t_store += wall_s() - t0, ++n_batches;
        if (fi.bad_record >= 0) return outside((long long)fi.bad_record, fi.bad_tid, fi.bad_pos, fi.reason) == 0;
        return true;
    });
    if (!fed) return 1;
    hpn_fixmate_result res;
    t0 = wall_s();
    rc = hpn_bam_fixmate_finish(ctx, &res);
    if (rc == HPN_E_NOMEM) return 1;
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_fixmate_finish");
    if (res.bad_record >= 0) return outside((long long)res.bad_record, res.bad_tid, res.bad_pos, res.reason);
    t_decide = wall_s() - t0;
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), -1, head_blocks)) return 1;
    BgzfWriter writer(-1);
    SliceRun run;
    const SliceCalls calls = {"hpn_bam_fixmate", hpn_bam_fixmate_emit, hpn_bam_fixmate_blocks, hpn_bam_fixmate_payload_dev, hpn_bam_fixmate_stored_dev};
    // (the output is a file: whenever the device's memory runs out it can go, and the host route makes it again)
    const int ws = write_slices(ctx, calls, res.n_out, -1, writer, false, [&]() {
        return writer.begin(o.out, head_blocks);
    }, run);
    if (ws == kSlicesNoOutput || ws == kSlicesNoMem) {   // the output so far goes; the host route makes it again, or says why it cannot
        if (run.created) writer.abandon(), unlink(o.out);
        return 1;
    }
    if (!writer.finish()) {
        fprintf(stderr, "[hpn] bam_fixmate: writing %s failed\n", o.out);
        leave(2);
    }
    fputs(said.c_str(), stderr);
    if (timing)
        fprintf(stderr, "[hpn] bam_fixmate: inflate + record index %.3f s, classify + store %.3f s, names + roles + order + patches %.3f s, "
                        "gather + patch + cuts + crc %.3f s, copies to the host %.3f s, handing to the writer %.3f s; %llu batches, %llu records in, %llu out, "
                        "%llu pairs, %llu singletons, %llu CT fields (%llu bytes), %llu blocks; writer: %.3f s deflating (all threads), %.3f s waited for\n",
                t_ingest, t_store, t_decide, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)n_batches, (unsigned long long)res.n_records,
                (unsigned long long)res.n_out, (unsigned long long)res.n_pairs, (unsigned long long)res.n_singletons, (unsigned long long)res.n_tags,
                (unsigned long long)res.bytes_added, (unsigned long long)run.n_blocks, writer.deflate_seconds(), writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    stamp("main");
    fixmate::Options o;
    if (!fixmate::parse_args(argc, argv, o)) return 1;
    const bool timing = getenv("HPN_TIMING") != nullptr;
    if (bam_gpu_enabled() && strcmp(o.in, "-") != 0 && strcmp(o.out, "-") != 0 && access(o.in, R_OK) == 0) {
        hpn_ctx *ctx = open_tool_ctx();
        stamp("context created");
        const int r = fixmate_device(ctx, o, timing);
        if (timing) fprintf(stderr, "[hpn] bam_fixmate: %s\n", r == 0 ? "device route" : "device route abandoned: host route");
        if (r == 0) {
            stamp("finished");
            quick_exit_ok();
        }
    } else if (timing) {
        fprintf(stderr, "[hpn] bam_fixmate: host route\n");
    }
    const int status = fixmate::fixmate_on_host(o);
    stamp("finished");
    leave(status);
}
