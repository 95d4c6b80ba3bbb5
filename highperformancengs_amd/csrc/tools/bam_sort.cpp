// bam_sort -- drop-in for `samtools sort` of the samtools-0.1.19 the reference vendors (bam_sort.c: bam_sort ->
// bam_sort_core_ext): the coordinate-sorted BAM every BAM tool here asks for, byte for byte samtools', with the keys, the sort,
// the gather into sorted order, the BGZF cuts and the CRC-32 of every block made on MI355X through libhpngs.
//
//   bam_sort [-n] [-f] [-o] [-l INT] [-@ INT] [-m INT[KMG]] <in.bam> <out.prefix>
//
// Writes <out.prefix>.bam (-f: <out.prefix>; -o: stdout).  Like the reference it says what went wrong on stderr and leaves with
// status 0; only fewer than two arguments are status 1.  No temporary file is written: where the reference would have sorted in
// chunks and merged them, the tool says "merging from N files" with the reference's N and writes at the default level, as the
// reference's merge step does whatever -l says.  The file is inflated and its records are indexed on the device as bamSplitChr's
// are; hpn_bam_sort_* keeps the records in a store on the device and hands the sorted output back slice by slice.  -n, a record
// with pos below -1 or above 2^30 - 2, a damaged or truncated file, an empty BGZF block in mid-file and a working set beyond
// the device's memory go to the sequential host route (host/bam_sort_host.hpp); HPN_BAM_GPU=0 selects it from the start.
// HPN_TIMING=1 says which route ran.
#include <sys/stat.h>

#include "../host/bam_tool.hpp"

using namespace hpn;

// 0 the output is written, 1 not for the device (the host route starts over; nothing has been said, no output is left)
static int sort_device(hpn_ctx *ctx, const bamsort::Options &o, bool timing)
{
    std::string said;
    bamsort::Header hdr;
    if (!open_bam_header(o.in, hdr, said)) return 1;   // on the host: its text changes, and its blocks are the writer's first
    bamsort::change_so(hdr.text, "coordinate");
    BgzfGpuStream bam;
    BamHeader parsed;
    if (!bam.open(ctx, o.in, parsed)) return 1;
    bam.start();
    int rc = hpn_bam_sort_begin(ctx);
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_sort_begin");
    double t_ingest = 0, t_store = 0, t_sort = 0, t0;
    uint64_t n_batches = 0;
    const bool fed = each_batch(bam, &t_ingest, [&](const BgzfDevice &) {
        hpn_bamsort_info si;
        t0 = wall_s();
        rc = hpn_bam_sort_add_raw_dev(ctx, bam.d_raw(), &si);
        if (rc == HPN_E_NOMEM) return false;               // the working set does not fit the device
        if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_sort_add_raw_dev");
        t_store += wall_s() - t0, ++n_batches;
        if (si.bad_record >= 0) {
            if (timing)
                fprintf(stderr, "[hpn] bam_sort: record %lld (refID %d, pos %d) is outside the device's domain (reason %u)\n", (long long)si.bad_record,
                        si.bad_tid, si.bad_pos, si.reason);
            return false;
        }
        return true;
    });
    if (!fed) return 1;
    hpn_bamsort_result res;
    t0 = wall_s();
    rc = hpn_bam_sort_finish(ctx, &res);
    if (rc == HPN_E_NOMEM) return 1;
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_sort_finish");
    if (res.bad_record >= 0) return 1;
    // the reference's file count: only an input that closes a first chunk needs the slots' history, which follows every chunk's
    // sorted order -- the whole file's order restricted to the chunk, since the sort is stable
    std::vector<uint64_t> parts;
    if (res.fresh_mem >= bamsort::max_mem_of(o)) {
        std::vector<uint32_t> sizes((size_t)res.n_records), order((size_t)res.n_records), rank((size_t)res.n_records), files;
        if ((rc = hpn_bam_sort_sizes(ctx, sizes.data(), res.n_records)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_sort_sizes");
        if ((rc = hpn_bam_sort_order(ctx, order.data(), res.n_records)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_sort_order");
        for (size_t j = 0; j < order.size(); ++j) rank[order[j]] = (uint32_t)j;
        std::vector<uint32_t>().swap(order);
        bamsort::plan_chunks(sizes.data(), sizes.size(), bamsort::max_mem_of(o), bamsort::threads_of(o),
                             [&](uint32_t a, uint32_t b) { return rank[a] < rank[b]; }, parts, files);
    }
    t_sort = wall_s() - t0;
    const int level = parts.empty() ? bamsort::level_of(o.level) : -1;
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), level, head_blocks)) return 1;
    const std::string path = bamsort::output_path(o);
    BgzfWriter writer(level);
    SliceRun run;
    const SliceCalls calls = {"hpn_bam_sort", hpn_bam_sort_emit, hpn_bam_sort_blocks, hpn_bam_sort_payload_dev, hpn_bam_sort_stored_dev};
    // (what has gone to stdout cannot be taken back: behind the first slice the device's memory running out is an error there)
    const int ws = write_slices(ctx, calls, res.n_records, level, writer, o.to_stdout, [&]() {
        fputs(said.c_str(), stderr);
        if (!parts.empty()) fprintf(stderr, "[bam_sort_core] merging from %d files...\n", (int)parts.size());
        if (!writer.begin(path.c_str(), head_blocks)) {
            if (!parts.empty()) fputs("[bam_merge_core2] fail to create the output file.\n", stderr);
            return false;
        }
        return true;
    }, run);
    if (ws == kSlicesNoOutput) return 0;
    if (ws == kSlicesNoMem) {   // the output so far goes; the host route makes it again
        if (run.created) writer.abandon();
        if (run.created && !o.to_stdout) unlink(path.c_str());
        return 1;
    }
    if (!writer.finish()) {
        fprintf(stderr, "bam_sort: writing %s failed\n", path.c_str());
        leave(2);
    }
    if (timing)
        fprintf(stderr, "[hpn] bam_sort: inflate + record index %.3f s, keys + store %.3f s, sort + offsets %.3f s, gather + cuts + crc %.3f s, copies to the host "
                        "%.3f s, handing to the writer %.3f s; %llu batches, %llu records, %u key bits, %llu blocks; writer: %.3f s deflating (all threads), "
                        "%.3f s waited for\n",
                t_ingest, t_store, t_sort, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)n_batches, (unsigned long long)res.n_records, res.sort_bits,
                (unsigned long long)run.n_blocks, writer.deflate_seconds(), writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    stamp("main");
    bamsort::Options o;
    if (!bamsort::parse_args(argc, argv, o)) return 1;
    const bool timing = getenv("HPN_TIMING") != nullptr;
    if (bam_gpu_enabled() && !o.by_name && strcmp(o.in, "-") != 0 && access(o.in, R_OK) == 0) {
        hpn_ctx *ctx = open_tool_ctx();
        stamp("context created");
        const int r = sort_device(ctx, o, timing);
        if (timing) fprintf(stderr, "[hpn] bam_sort: %s\n", r == 0 ? "device route" : "device route abandoned: host route");
        if (r == 0) {
            stamp("finished");
            quick_exit_ok();
        }
    } else if (timing) {
        fprintf(stderr, "[hpn] bam_sort: host route\n");
    }
    const int status = bamsort::sort_on_host(o);
    stamp("finished");
    leave(status);
}
