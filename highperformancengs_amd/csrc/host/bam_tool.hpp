// bam_tool.hpp -- what the BAM tools over a device session do alike: the header read on the host (bam_sort, bam_rmdup), the
// loop over the stream's batches (those two and bam_index), and the way from a session's slices to the BGZF writer (the two).
#pragma once
#include "bam_gpu.hpp"
#include "bam_sort_host.hpp"
#include "report.hpp"

namespace hpn {

// The header as the writer needs it; what bam_header_read would remark goes to `said`, for the tool to say when nothing can send
// the file to the host route any more.  false: not for the device.
inline bool open_bam_header(const char *path, bamsort::Header &hdr, std::string &said)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    if (!bai::has_eof_marker(f)) said += "[bam_header_read] EOF marker is absent. The input is probably truncated.\n";
    bai::BgzfSeq z(f);
    const int hr = bamsort::read_header(z, hdr);
    fclose(f);
    return hr == 0;
}

// Every batch of the stream that holds records goes to batch(device), which says whether to go on.  false: not for the device
// (a damaged file, an empty BGZF block in mid-file, or batch said so).  *t_ingest: seconds waited for the batches.
template <class Batch>
inline bool each_batch(BgzfGpuStream &bam, double *t_ingest, Batch &&batch)
{
    bool empty_seen = false;
    for (;;) {
        hpn_raw_info info;
        const double t0 = wall_s();
        const int r = bam.next(&info);
        *t_ingest += wall_s() - t0;
        if (r < 0) return false;
        if (r == 0) return true;
        const BgzfDevice &dev = bam.device();
        if (!dev.n_blocks()) continue;
        // a block of no bytes ends the stream for samtools' reader: only the file's last block may be one
        if (empty_seen || dev.empty_blocks() > 1 || (dev.empty_blocks() == 1 && !dev.last_block_empty())) return false;
        empty_seen = dev.empty_blocks() != 0;
        if (!info.n_records) continue;
        if (!batch(dev)) return false;
    }
}

#ifdef HPN_TEST_HOOKS
static const uint64_t kSliceRecords = 1000;        // (the test-hooks build: the open block is carried over many slices)
#else
static const uint64_t kSliceRecords = 1u << 22;    // ~1 GB of payload per slice at 250 bytes a record
#endif

struct SliceCalls {        // a family's name (hpn_bam_sort, ...) and its _emit, _blocks, _payload_dev, _stored_dev
    std::string name;
    int (*emit)(hpn_ctx *, uint64_t, uint64_t, int, hpn_split_info *);
    int (*blocks)(hpn_ctx *, uint64_t, hpn_split_block *, uint64_t, uint64_t *);
    int (*payload_dev)(hpn_ctx *, const uint8_t **, uint64_t *);
    int (*stored_dev)(hpn_ctx *, const uint8_t **, uint64_t *);
};

struct SliceRun {
    double t_emit = 0, t_copy = 0, t_hand = 0;
    uint64_t n_blocks = 0;
    bool created = false;  // the output exists
};
enum { kSlicesDone = 0, kSlicesNoMem, kSlicesNoOutput };

// The session's n_out records, slice by slice: emitted, copied to the host, handed to the writer (level 0: the stored image as
// the device framed it).  create() makes the output behind the first slice -- everything the device needs has been allocated by
// then -- and says whether it exists.  kSlicesNoMem: the device's memory ran out; with keep_once_created not once the output exists.
template <class Create>
inline int write_slices(hpn_ctx *ctx, const SliceCalls &f, uint64_t n_out, int level, BgzfWriter &writer, bool keep_once_created, Create &&create,
                        SliceRun &run)
{
    std::vector<hpn_split_block> blocks;
    std::vector<uint8_t> bytes;
    int rc;
    for (uint64_t first = 0;;) {
        const uint64_t cnt = n_out - first < kSliceRecords ? n_out - first : kSliceRecords;
        const bool last = first + cnt == n_out;
        hpn_split_info si;
        double t0 = wall_s();
        rc = f.emit(ctx, first, cnt, last ? 1 : 0, &si);
        if (rc == HPN_E_NOMEM && !(run.created && keep_once_created)) return kSlicesNoMem;
        if (rc != HPN_OK) die_hpn(ctx, rc, (f.name + "_emit").c_str());
        run.t_emit += wall_s() - t0, t0 = wall_s();
        uint64_t nb = 0, n = 0;
        const uint8_t *d = nullptr;
        blocks.resize(si.n_blocks);
        if ((rc = f.blocks(ctx, 0, blocks.data(), blocks.size(), &nb)) != HPN_OK) die_hpn(ctx, rc, (f.name + "_blocks").c_str());
        rc = level == 0 ? f.stored_dev(ctx, &d, &n) : f.payload_dev(ctx, &d, &n);
        if (rc != HPN_OK) die_hpn(ctx, rc, (f.name + "_payload_dev").c_str());
        bytes.resize(n);
        if (n && ((rc = hpn_memcpy_d2h(ctx, bytes.data(), d, n)) != HPN_OK || (rc = hpn_ctx_sync(ctx)) != HPN_OK)) die_hpn(ctx, rc, "hpn_memcpy_d2h");
        run.t_copy += wall_s() - t0, t0 = wall_s();
        if (!run.created) {
            if (!create()) return kSlicesNoOutput;
            run.created = true;
        }
        if (level == 0) writer.add_framed(bytes.data(), (size_t)n);
        else
            for (size_t k = 0; k < nb; ++k) writer.add(bytes.data() + blocks[k].off, blocks[k].len, blocks[k].crc, true);
        run.n_blocks += nb;
        run.t_hand += wall_s() - t0;
        first += cnt;
        if (last) return kSlicesDone;
    }
}

}  // namespace hpn
