// text_feed.hpp -- one FASTQ file into a tool's sink as raw text, through the input routes that gzfastq_sample, gzfastq_uniq
// and gzfastq_sort share:
//   bgzip                the blocks inflated on the device (host/bam_gpu.hpp), the text handed on where it lies
//   one-member gzip      stretches inflated on the device (host/gz_gpu.hpp), likewise
//   anything else        read -- and, where compressed, inflated -- by the host's reader threads (TextPump)
// A device route that cannot open its stream leaves the file to the next one.  The sink (no base class: a small struct per tool) has
//   void route_begins()                                    a route's stream has opened; nothing has been delivered yet
//   bool chunk(const void *text, uint64_t n, bool last)    host or device text, cut anywhere; false: the text is not regular
//   bool start_over()                                      a device route gave up after it had delivered text: true when what
//                                                          the sink took has been dropped and the next route may begin again
// (fastq_count and fastq_trim have cascades of their own: the tally fetch and the sharded lanes there, the carried bytes and
// the output that cannot be rewound here.)
#pragma once
#include "bam_gpu.hpp"
#include "gz_gpu.hpp"
#include "report.hpp"
#include "tally_stream.hpp"
#include "text_stream.hpp"

namespace hpn {

// kIrregular: the text is not regular FASTQ (or a route gave up and the sink could not start over) -- nothing the sink took
// counts and the caller frames the file on the host.  kDamaged: the host's reader met a CRC-32 / ISIZE / data error.
enum class FeedEnd { kDone, kIrregular, kDamaged };

// text on the device, in slices (each framed by one call)
template <class Sink>
bool feed_device_text(Sink &sink, const uint8_t *d_text, uint64_t total, bool fin)
{
    const uint64_t slice = text_slice_bytes((uint64_t)32 << 20);
    for (uint64_t at = 0; at < total || (fin && total == 0);) {
        const uint64_t k = total - at < slice ? total - at : slice;
        if (!sink.chunk(d_text + at, k, fin && at + k == total)) return false;
        at += k;
        if (total == 0) break;
    }
    return true;
}

template <class Sink>
FeedEnd feed_fastq_file(hpn_ctx *ctx, const char *path, const char *tool, Sink &sink)
{
    if (bam_gpu_enabled() && !test_env("HPN_NO_BGZF") && is_bgzf_file(path)) {   // bgzip: the blocks are inflated on the GPU
        BgzfGpuStream gs;
        if (gs.open_text(ctx, path)) {
            sink.route_begins();
            for (;;) {
                hpn_raw_info bi;
                const int r = gs.next(&bi);
                if (r < 0) break;
                const bool fin = r == 0 || gs.at_eof();
                if (!feed_device_text(sink, gs.d_raw(), r == 0 ? 0 : bi.n_records, fin)) return FeedEnd::kIrregular;   // text mode: n_records = bytes inflated
                if (fin) return FeedEnd::kDone;
            }
            if (!sink.start_over()) return FeedEnd::kIrregular;
        }
    }
    if (gz_gpu_route_wanted() && is_plain_gzip_file(path)) {   // gzip members inflated on the GPU in stretches
        GzGpuStream gs;
        if (open_gz_gpu_stream(gs, ctx, path)) {
            sink.route_begins();
            for (;;) {
                uint64_t n = 0;
                const int r = gs.next(&n);
                if (r < 0) break;
                const bool fin = r == 0 || gs.at_end();
                if (!feed_device_text(sink, gs.d_text(), n, fin)) return FeedEnd::kIrregular;
                if (fin) return FeedEnd::kDone;
            }
            if (!sink.start_over()) return FeedEnd::kIrregular;
        }
    }
    // text read (and, where compressed, inflated) by the host's reader threads, framed on the device
    TextPump pump(ctx, path, text_chunk_bytes());
    if (!pump.ok()) die_hpn(ctx, HPN_E_NOMEM, tool);
    sink.route_begins();
    TextPump::Chunk c;
    while (pump.next(c)) {
        const bool ok = sink.chunk(c.p, c.n, c.eof);
        pump.recycle(c);
        if (!ok) return FeedEnd::kIrregular;
    }
    return pump.damaged() ? FeedEnd::kDamaged : FeedEnd::kDone;
}

}  // namespace hpn
