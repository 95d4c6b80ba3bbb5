// bam_index -- drop-in for `samtools index` of the samtools-0.1.19 the reference vendors (bam_index.c: bam_index ->
// bam_index_build2 -> bam_index_core / bam_index_save): the .bai every BAM tool here asks for, byte for byte samtools', with the
// pass over the records made on MI355X through libhpngs.
//
//   bam_index <in.bam> [out.index]            (default: <in.bam>.bai)
//
// Like the reference it says what went wrong on stderr and leaves with status 0 whether or not an index was written; only the
// missing argument is status 1.  The file is inflated and its records are indexed on the device as bamSplitChr's are (read-ahead,
// batches); hpn_bam_bai_* turns every batch into run heads, counts and the linear index.  A file outside the device's domain --
// records out of order, a window beyond its target, a CIGAR `B`, an empty BGZF block in mid-file, a damaged or truncated file --
// is indexed by the sequential host route (host/bai_build.hpp), which follows the reference everywhere, messages included;
// HPN_BAM_GPU=0 selects that route from the start.  HPN_TIMING=1 says which route ran.
#include <sys/stat.h>

#include "../host/bam_tool.hpp"

using namespace hpn;

// 0 the index is in `ix`, 1 not for the device (the host route starts over; nothing has been said or written)
static int index_device(hpn_ctx *ctx, const char *path, bai::Index &ix, std::string &said, bool timing)
{
    struct stat sb;
    if (stat(path, &sb) != 0) return 1;
    const uint64_t file_size = (uint64_t)sb.st_size;
    {   // bam_header_read looks for the EOF marker first and only remarks on its absence
        FILE *f = fopen(path, "rb");
        if (!f) return 1;
        if (!bai::has_eof_marker(f)) said += "[bam_header_read] EOF marker is absent. The input is probably truncated.\n";
        fclose(f);
    }
    BgzfGpuStream bam;
    BamHeader hdr;
    if (!bam.open(ctx, path, hdr)) return 1;
    const int32_t n_ref = hdr.n_targets();
    std::vector<int32_t> target_len((size_t)n_ref);
    uint64_t windows = 0;
    for (int32_t t = 0; t < n_ref; ++t) {
        target_len[(size_t)t] = (int32_t)hdr.target_len[(size_t)t];
        if (target_len[(size_t)t] > 0) windows += (uint64_t)((target_len[(size_t)t] - 1) >> 14) + 1;
    }
    if (windows > ((uint64_t)1 << 27)) return 1;
    bam.start();
    int rc = hpn_bam_bai_begin(ctx, n_ref, target_len.data(), bam.first_voffset());
    if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_bam_bai_begin");
    double t_ingest = 0, t_index = 0, t0;
    uint64_t n_batches = 0, n_runs = 0;
    std::vector<uint64_t> addr;
    const bool fed = each_batch(bam, &t_ingest, [&](const BgzfDevice &dev) {
        addr.resize(dev.n_blocks() + 1);
        for (size_t k = 0; k <= dev.n_blocks(); ++k) addr[k] = bam.batch_file_offset() + dev.block_rel()[k];
        hpn_bai_info bi;
        t0 = wall_s();
        if ((rc = hpn_bam_bai_add_raw_dev(ctx, bam.d_raw(), dev.d_blocks(), dev.n_blocks(), addr.data(), 0, 0, &bi)) != HPN_OK)
            die_hpn(ctx, rc, "hpn_bam_bai_add_raw_dev");
        t_index += wall_s() - t0, ++n_batches, n_runs += bi.n_runs;
        if (bi.bad_record >= 0) {
            if (timing)
                fprintf(stderr, "[hpn] bam_index: record %lld (refID %d, pos %d) is outside the device's domain (reason %u)\n", (long long)bi.bad_record, bi.bad_tid,
                        bi.bad_pos, bi.reason);
            return false;
        }
        return true;
    });
    if (!fed) return 1;
    if (!bam.plain_headers()) return 1;
    hpn_bai_info bi;
    if ((rc = hpn_bam_bai_add_raw_dev(ctx, nullptr, nullptr, 0, nullptr, 1, file_size << 16, &bi)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_bai_add_raw_dev");
    hpn_bai_result res;
    t0 = wall_s();
    if ((rc = hpn_bam_bai_finish(ctx, &res)) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_bai_finish");
    std::vector<hpn_bai_target> targets((size_t)n_ref);
    std::vector<hpn_bai_chunk> chunks((size_t)res.n_chunks);
    std::vector<uint64_t> lin((size_t)res.n_windows);
    if ((rc = hpn_bam_bai_read(ctx, targets.data(), chunks.data(), lin.data())) != HPN_OK) die_hpn(ctx, rc, "hpn_bam_bai_read");
    const double t_finish = wall_s() - t0;
    // the file's order: a target's bins as their first chunk closed -- the chunks of a bin are in file order, so that is the order
    // of the bins' first offsets --, the metadata bin behind them
    ix.t.assign((size_t)n_ref, bai::TargetIndex());
    ix.n_no_coor = res.n_no_coor;
    for (int32_t t = 0; t < n_ref; ++t) {
        const hpn_bai_target &ht = targets[(size_t)t];
        bai::TargetIndex &ti = ix.t[(size_t)t];
        for (uint64_t k = ht.first_chunk; k < ht.first_chunk + ht.n_chunks; ++k) {
            if (ti.bins.empty() || ti.bins.back().first != chunks[(size_t)k].bin) ti.bins.emplace_back(chunks[(size_t)k].bin, std::vector<bai::Chunk>());
            ti.bins.back().second.push_back(bai::Chunk{chunks[(size_t)k].beg, chunks[(size_t)k].end});
        }
        std::stable_sort(ti.bins.begin(), ti.bins.end(), [](const std::pair<uint32_t, std::vector<bai::Chunk>> &a,
                                                           const std::pair<uint32_t, std::vector<bai::Chunk>> &b) { return a.second[0].beg < b.second[0].beg; });
        if (ht.has_records)
            ti.bins.emplace_back(bai::kMetaBin, std::vector<bai::Chunk>{bai::Chunk{ht.off_beg, ht.off_end}, bai::Chunk{ht.n_mapped, ht.n_unmapped}});
        ti.n_lin = ht.n_windows;
        ti.lin.assign(lin.begin() + (size_t)ht.first_window, lin.begin() + (size_t)(ht.first_window + (uint64_t)ht.n_windows));
    }
    if (timing)
        fprintf(stderr, "[hpn] bam_index: inflate + record index %.3f s, per-record pass + run heads %.3f s, lists + linear index %.3f s; %llu batches, "
                        "%llu records, %llu runs, %llu chunks\n",
                t_ingest, t_index, t_finish, (unsigned long long)n_batches, (unsigned long long)res.n_records, (unsigned long long)n_runs,
                (unsigned long long)res.n_chunks);
    return 0;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    stamp("main");
    if (argc < 2) {
        fprintf(stderr, "Usage: samtools index <in.bam> [out.index]\n");
        return 1;
    }
    const char *in = argv[1], *out = argc >= 3 ? argv[2] : nullptr;
    const bool timing = getenv("HPN_TIMING") != nullptr;
    int r = 1;
    if (bam_gpu_enabled() && access(in, R_OK) == 0) {
        hpn_ctx *ctx = open_tool_ctx();
        stamp("context created");
        bai::Index ix;
        std::string said;
        r = index_device(ctx, in, ix, said, timing);
        if (timing) fprintf(stderr, "[hpn] bam_index: %s\n", r == 0 ? "device route" : "device route abandoned: host route");
        if (r == 0) {
            fputs(said.c_str(), stderr);
            (void)bai::save_index(ix, in, out);
            stamp("finished");
            quick_exit_ok();
        }
    } else if (timing) {
        fprintf(stderr, "[hpn] bam_index: host route\n");
    }
    const int status = bai::index_on_host(in, out);
    stamp("finished");
    leave(status);
}
