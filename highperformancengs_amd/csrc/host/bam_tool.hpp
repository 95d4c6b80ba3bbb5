// bam_tool.hpp -- what the BAM tools over a device session do alike: the header read on the host, the loop over the stream's
// batches (bam_index too), and for the record-store sessions (bam_sort, bam_rmdup, bam_merge, bam_fixmate, bam_view) the batches into the
// session, its _finish, the way from its slices to the BGZF writer, and main()'s choice between the device and the host route.
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

struct SliceCalls {        // a family's name (hpn_bam_sort, ...), its tool's, and its _emit, _blocks, _payload_dev, _stored_dev
    std::string name;
    const char *tool;
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

struct FeedRun {
    double t_ingest = 0, t_store = 0;      // seconds waited for the batches, seconds in _add_raw_dev
    uint64_t n_batches = 0;
};

// (with HPN_TIMING: why the device route ends here; r: a family's info or result)
template <class R>
inline void say_outside(const char *tool, bool timing, const R &r)
{
    if (timing)
        fprintf(stderr, "[hpn] %s: record %lld (refID %d, pos %d) is outside the device's domain (reason %u)\n", tool, (long long)r.bad_record, r.bad_tid, r.bad_pos,
                r.reason);
}

// Every batch of the stream into the session by the family's _add_raw_dev.  false: not for the device (each_batch's reasons, a
// working set beyond the device's memory, a record outside the family's domain).
template <class Info>
inline bool feed_session(hpn_ctx *ctx, BgzfGpuStream &bam, const SliceCalls &f, int (*add)(hpn_ctx *, const uint8_t *, Info *), bool timing, FeedRun &run)
{
    return each_batch(bam, &run.t_ingest, [&](const BgzfDevice &) {
        Info info;
        const double t0 = wall_s();
        const int rc = add(ctx, bam.d_raw(), &info);
        if (rc == HPN_E_NOMEM) return false;               // the working set does not fit the device
        if (rc != HPN_OK) die_hpn(ctx, rc, (f.name + "_add_raw_dev").c_str());
        run.t_store += wall_s() - t0, ++run.n_batches;
        if (info.bad_record < 0) return true;
        say_outside(f.tool, timing, info);
        return false;
    });
}

// The family's _finish.  false: not for the device (its memory ran out, or a record only _finish can find lies outside the domain:
// rmdup's and fixmate's do, and say so; sort's and merge's find none of their own, and a session feed_session saw die never comes
// here, so for those two the line below cannot be reached and their messages are what they were).
template <class Result>
inline bool finish_session(hpn_ctx *ctx, const SliceCalls &f, int (*finish)(hpn_ctx *, Result *), bool timing, Result &res)
{
    const int rc = finish(ctx, &res);
    if (rc == HPN_E_NOMEM) return false;
    if (rc != HPN_OK) die_hpn(ctx, rc, (f.name + "_finish").c_str());
    if (res.bad_record < 0) return true;
    say_outside(f.tool, timing, res);
    return false;
}

// The finished session's n_out records behind the header's plain blocks, to the writer's end.  create(head_blocks) is
// write_slices' create().  kSlicesDone: `path` is written.  kSlicesNoOutput: create() said no.  kSlicesNoMem: not for the device,
// and what was written is gone -- unless it went to stdout, where the device's memory running out behind the first slice is an
// error (what has gone there cannot be taken back).  A write that fails ends the tool: "<says>: writing <path> failed", status 2.
template <class Create>
inline int write_session(hpn_ctx *ctx, const SliceCalls &f, const bamsort::Header &hdr, uint64_t n_out, int level, BgzfWriter &writer, const char *path,
                         bool to_stdout, const char *says, Create &&create, SliceRun &run)
{
    const std::vector<uint8_t> head = hdr.bytes();
    std::vector<uint8_t> head_blocks;
    if (!bgzf_plain_blocks(head.data(), head.size(), level, head_blocks)) return kSlicesNoMem;
    const int ws = write_slices(ctx, f, n_out, level, writer, to_stdout, [&]() { return create(head_blocks); }, run);
    if (ws == kSlicesNoMem) {   // the output so far goes; the host route makes it again
        if (run.created) writer.abandon();
        if (run.created && !to_stdout) unlink(path);
    }
    if (ws != kSlicesDone) return ws;
    if (!writer.finish()) {
        fprintf(stderr, "%s: writing %s failed\n", says, path);
        leave(2);
    }
    return kSlicesDone;
}

// main() of a tool with a device and a host route.  parse(): the arguments, not 0: main's status at once.  eligible(): the job is
// the device's to try.  on_device(ctx, timing): 0 the output is written, 1 not for the device -- the host route starts over --,
// 2 the job has ended with the reference's status 1.  on_host(): the host route's status.  HPN_TIMING says which route ran.
template <class Parse, class Eligible, class Device, class Host>
inline int run_tool(const char *tool, Parse &&parse, Eligible &&eligible, Device &&on_device, Host &&on_host)
{
    bind_before_runtime();
    stamp("main");
    const int early = parse();
    if (early) return early;
    const bool timing = getenv("HPN_TIMING") != nullptr;
    if (eligible()) {
        hpn_ctx *ctx = open_tool_ctx();
        stamp("context created");
        const int r = on_device(ctx, timing);
        if (timing) fprintf(stderr, "[hpn] %s: %s\n", tool, r != 1 ? "device route" : "device route abandoned: host route");
        if (r == 0) {
            stamp("finished");
            quick_exit_ok();
        }
        if (r == 2) leave(1);
    } else if (timing) {
        fprintf(stderr, "[hpn] %s: host route\n", tool);
    }
    const int status = on_host();
    stamp("finished");
    leave(status);
}

}  // namespace hpn
