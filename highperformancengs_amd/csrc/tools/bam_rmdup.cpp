// bam_rmdup -- drop-in for `samtools rmdup` of the samtools-0.1.19 the reference vendors (bam_rmdup.c: bam_rmdup ->
// bam_rmdup_core / bam_rmdupse_core): a coordinate-sorted BAM without its PCR duplicates, byte for byte samtools', with its
// messages and status; the decisions, the gather of the survivors, the BGZF cuts and the CRC-32 of every block made on MI355X
// through libhpngs.
//
//   bam_rmdup [-sS] <input.srt.bam> <output.bam>
//
// The file is inflated and its records are indexed on the device as bam_sort's are; hpn_bam_rmdup_* classifies every record,
// keeps the records in a store on the device and hands the output back slice by slice.  -s and -S, a header that is not parsed
// in silence, a file that is not sorted or begins with unplaced records, an RG tag that is no string, aux fields outside the
// format, an inconsistent pair, a damaged or truncated file and a working set beyond the device's memory go to the sequential
// host route (host/bam_rmdup_host.hpp); HPN_BAM_GPU=0 selects it from the start.  HPN_TIMING=1 says which route ran.
#include <sys/stat.h>

#include <algorithm>

#include "../host/bam_rmdup_host.hpp"
#include "../host/bam_tool.hpp"

using namespace hpn;

static const SliceCalls kCalls = {"hpn_bam_rmdup", "bam_rmdup", hpn_bam_rmdup_emit, hpn_bam_rmdup_blocks, hpn_bam_rmdup_payload_dev, hpn_bam_rmdup_stored_dev};

// 0 the output is written, 1 not for the device (the host route starts over; nothing has been said, no output is left)
static int rmdup_device(hpn_ctx *ctx, const rmdup::Options &o, bool timing)
{
    std::string said;
    bamsort::Header hdr;
    if (!open_bam_header(o.in, hdr, said)) return 1;   // on the host: its blocks are the writer's first, its @RG lines the device's table
    std::map<std::string, std::string> tbl;
    if (!rmdup::id_table(hdr.text, tbl)) return 1;
    std::vector<std::string> lib_name(1, "\t");       // library 0: no RG, an unknown ID, no LB
    std::vector<const char *> ids;
    std::vector<uint32_t> lib_of_id;
    for (const auto &kv : tbl) {
        if (kv.first.find('\0') != std::string::npos) return 1;
        size_t l = std::find(lib_name.begin() + 1, lib_name.end(), kv.second) - lib_name.begin();
        if (kv.second == "\t") l = 0;
        if (l == lib_name.size()) lib_name.push_back(kv.second);
        ids.push_back(kv.first.c_str()), lib_of_id.push_back((uint32_t)l);
    }
    BgzfGpuStream bam;
    BamHeader parsed;
    if (!bam.open(ctx, o.in, parsed)) return 1;
    bam.start();
    int rc = hpn_bam_rmdup_begin(ctx, (int32_t)hdr.name.size(), (uint32_t)ids.size(), ids.data(), lib_of_id.data(), (uint32_t)lib_name.size());
    if (rc == HPN_E_ARG || rc == HPN_E_NOMEM) return 1;       // (more IDs than the table takes)
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_rmdup_begin");
    FeedRun fed;
    if (!feed_session(ctx, bam, kCalls, hpn_bam_rmdup_add_raw_dev, timing, fed)) return 1;
    hpn_rmdup_result res;
    const double t0 = wall_s();
    if (!finish_session(ctx, kCalls, hpn_bam_rmdup_finish, timing, res)) return 1;
    std::vector<hpn_rmdup_lib> libs(lib_name.size());
    std::vector<hpn_rmdup_target> targets(hdr.name.size() + 1);
    if ((rc = hpn_bam_rmdup_counts(ctx, libs.data(), targets.data())) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_rmdup_counts");
    const double t_decide = wall_s() - t0;
    BgzfWriter writer(-1);
    SliceRun run;
    // (the output is a file: whenever the device's memory runs out it can go, and the host route makes it again)
    const int ws = write_session(ctx, kCalls, hdr, res.n_out, -1, writer, o.out, false, "[hpn] bam_rmdup", [&](const std::vector<uint8_t> &head_blocks) {
        if (!writer.begin(o.out, head_blocks)) {
            fputs(said.c_str(), stderr);
            fputs("[bam_rmdup] fail to read/write input files\n", stderr);
            leave(1);
        }
        return true;
    }, run);
    if (ws != kSlicesDone) return 1;
    // the reference's words, now that nothing can send the file to the host any more: per target that has records what the
    // target before left in the set, then "processing reference"; the same check where the unplaced records begin; the libraries
    // in the order of khash's buckets, entered as their first heads came
    fputs(said.c_str(), stderr);
    uint64_t pending = 0;
    for (size_t t = 0; t < targets.size(); ++t) {
        if (!targets[t].has_records) continue;
        if (pending) fprintf(stderr, "[bam_rmdup_core] %llu unmatched pairs\n", (unsigned long long)pending);
        if (t < hdr.name.size()) fprintf(stderr, "[bam_rmdup_core] processing reference %s...\n", hdr.name[t].c_str());
        pending = targets[t].unmatched;
    }
    std::vector<std::pair<int64_t, size_t>> by_first;
    std::map<std::string, rmdup::LibCount> counts;
    for (size_t l = 0; l < libs.size(); ++l)
        if (libs[l].first >= 0) {
            by_first.emplace_back(libs[l].first, l);
            counts[lib_name[l]].checked = libs[l].checked, counts[lib_name[l]].removed = libs[l].removed;
        }
    std::sort(by_first.begin(), by_first.end());
    std::vector<std::string> seen;
    for (const auto &f : by_first) seen.push_back(lib_name[f.second]);
    rmdup::library_lines("bam_rmdup_core", counts, seen);
    if (timing)
        fprintf(stderr, "[hpn] bam_rmdup: inflate + record index %.3f s, classify + store %.3f s, groups + names + placement %.3f s, gather + cuts + crc %.3f s, "
                        "copies to the host %.3f s, handing to the writer %.3f s; %llu batches, %llu records in, %llu heads, %llu records out, %llu blocks; "
                        "writer: %.3f s deflating (all threads), %.3f s waited for\n",
                fed.t_ingest, fed.t_store, t_decide, run.t_emit, run.t_copy, run.t_hand, (unsigned long long)fed.n_batches, (unsigned long long)res.n_records,
                (unsigned long long)res.n_heads, (unsigned long long)res.n_out, (unsigned long long)run.n_blocks, writer.deflate_seconds(), writer.waited_seconds());
    return 0;
}

int main(int argc, char *argv[])
{
    rmdup::Options o;
    return run_tool(
        "bam_rmdup",
        [&]() { return rmdup::parse_args(argc, argv, o) ? 0 : 1; },
        [&]() {
            return bam_gpu_enabled() && !o.se && strcmp(o.in, "-") != 0 && strcmp(o.out, "-") != 0 && access(o.in, R_OK) == 0;
        },
        [&](hpn_ctx *ctx, bool timing) { return rmdup_device(ctx, o, timing); },
        [&]() { return rmdup::rmdup_on_host(o); });
}
