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

static const SliceCalls kCalls = {"hpn_bam_sort", "bam_sort", hpn_bam_sort_emit, hpn_bam_sort_blocks, hpn_bam_sort_payload_dev, hpn_bam_sort_stored_dev};

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
    FeedRun fed;
    if (!feed_session(ctx, bam, kCalls, hpn_bam_sort_add_raw_dev, timing, fed)) return 1;
    hpn_bamsort_result res;
    const double t0 = wall_s();
    if (!finish_session(ctx, kCalls, hpn_bam_sort_finish, timing, res)) return 1;
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
    const double t_sort = wall_s() - t0;
    const int level = parts.empty() ? bamsort::level_of(o.level) : -1;
    const std::string path = bamsort::output_path(o);
    BgzfWriter writer(level);
    SliceRun run;
    const int ws = write_session(ctx, kCalls, hdr, res.n_records, level, writer, path.c_str(), o.to_stdout, "bam_sort", [&](const std::vector<uint8_t> &head_blocks) {
        fputs(said.c_str(), stderr);
        if (!parts.empty()) fprintf(stderr, "[bam_sort_core] merging from %d files...\n", (int)parts.size());
        if (!writer.begin(path.c_str(), head_blocks)) {
            if (!parts.empty()) fputs("[bam_merge_core2] fail to create the output file.\n", stderr);
            return false;
        }
        return true;
    }, run);
    if (ws == kSlicesNoMem) return 1;
    if (ws == kSlicesNoOutput) return 0;
    if (timing)
        fprintf(stderr, "[hpn] bam_sort: inflate + record index %.3f s, keys + store %.3f s, sort + offsets %.3f s, gather + cuts + crc %.3f s, copies to the host "
                        "%.3f s, handing to the writer %.3f s; %llu batches, %llu records, %u key bits, %llu blocks; writer: %.3f s deflating (all threads), "
                        "%.3f s waited for\n",
                fed.t_ingest, fed.t_store, t_sort, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)fed.n_batches, (unsigned long long)res.n_records, res.sort_bits,
                (unsigned long long)run.n_blocks, writer.deflate_seconds(), writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    bamsort::Options o;
    return run_tool(
        "bam_sort",
        [&]() { return bamsort::parse_args(argc, argv, o) ? 0 : 1; },
        [&]() {
            return bam_gpu_enabled() && !o.by_name && strcmp(o.in, "-") != 0 && access(o.in, R_OK) == 0;
        },
        [&](hpn_ctx *ctx, bool timing) { return sort_device(ctx, o, timing); },
        [&]() { return bamsort::sort_on_host(o); });
}
