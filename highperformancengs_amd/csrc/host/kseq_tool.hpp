// kseq_tool.hpp -- the main of map_kseq and kbtree_kseq: one positional argument, a plain or gzip FASTA / FASTQ file ("-" or an
// empty name: standard input), read as the reference's kseq_read reads it; the first record of every distinct sequence, in the
// sequences' order, as "name comment\nseq\n+\nqual\n" on stdout and the number of distinct sequences on stderr.
//
// The text goes to the device through the feed the store tools share (text_feed.hpp, store_tool.hpp) and is framed, ordered and
// formatted there (hpn_kseq_*); text that has neither of the two shapes the device frames is read by host/kseq_read.hpp and
// finished through a std::map.  Status 2 where the reference has no answer: a NUL byte in the text (its "%s" cuts the line
// there), a damaged gzip stream, an input beyond the device's memory -- and for kbtree_kseq sequences of more than one length,
// where what the reference's B-tree holds is an artefact of its comparison's missing parentheses.
#pragma once
#include <fcntl.h>

#include <string>

#include "kseq_read.hpp"
#include "store_tool.hpp"

namespace hpn {

[[noreturn]] inline void kseq_mixed_lengths(const char *tool, const char *path, unsigned long long a, unsigned long long b)
{
    fprintf(stderr,
            "%s: %s: sequences of %llu and of %llu bytes (the reference has no answer there: with sequences of more than one length its "
            "B-tree's comparison is true both ways)\n",
            tool, path, a, b);
    leave(2);
}

inline int kseq_tool_main(int argc, char *argv[], const char *tool, bool btree)
{
    bind_before_runtime();
    if (argc < 2) {
        fprintf(stderr,
                "\nUsage: %s <in.fa|in.fq|in.gz|->\n"
                "  Reads FASTA or FASTQ (plain or gzip; wrapped lines, CRLF) and prints the first record of every distinct\n"
                "  sequence, in the order of the sequences, as \"name comment\\nseq\\n+\\nqual\\n\"; the number of distinct\n"
                "  sequences goes to stderr (MI355X build of HighPerformanceNGS %s).\n\n",
                argv[0], tool);
        exit(1);
    }
    const char *path = argv[1];
    const bool is_stdin = strncmp(path, "-", 1) == 0 || !strcmp(path, "");
    if (!is_stdin) {   // the reference opens with O_CREAT: a missing file is made, and is empty
        const int fd = ::open(path, O_CREAT | O_RDONLY, 0666);
        if (fd >= 0) ::close(fd);
        else fprintf(stderr, "Failed to create input file (%s)", path);
    }
    hpn_ctx *ctx = open_tool_ctx();
    int rc;
    const long long begin = usec();
    std::string mem;
    bool done = false, nul = false;
    auto add = [&](const void *text, uint64_t n, bool last) {
        hpn_sort_info si = {};
        const int arc = hpn_kseq_add(ctx, text, n, last, &si);
        if (si.irregular & HPN_TEXT_NUL) nul = true;
        return chunk_taken(ctx, tool, "hpn_kseq_add", arc, si.irregular);
    };
    if (is_stdin) slurp_or_refuse(tool, path, mem);
    if (text_path_enabled()) {
        if ((rc = hpn_kseq_begin(ctx, 0)) != HPN_OK) die_hpn(ctx, rc, "hpn_kseq_begin");
        done = is_stdin ? memory_feed(mem, add) : device_feed(ctx, tool, path, add);
    }
    if (nul) refuse(tool, path, "NUL byte in the text");
    const long long fed = usec();
    if (done) {
        static hpn_kseq_result res;
        if ((rc = hpn_kseq_finish(ctx, &res)) != HPN_OK) die_hpn(ctx, rc, "hpn_kseq_finish");
        if (btree && !res.one_length) kseq_mixed_lengths(tool, path, res.first_len, res.other_len);
        fprintf(stderr, "%llu\n", (unsigned long long)res.n_distinct);
        const long long ordered = usec();
        write_device_output(ctx, tool, "-", "", res.out_bytes, text_slice_bytes((uint64_t)32 << 20), [&](uint64_t at, void *buf, uint64_t cap, uint64_t *got) {
            const int wrc = hpn_kseq_write(ctx, at, buf, cap, got);
            if (wrc != HPN_OK) die_hpn(ctx, wrc, "hpn_kseq_write");
        });
        if (getenv("HPN_TIMING"))
            fprintf(stderr,
                    "[hpn] kseq: route device, shape %s, %llu records; reading and framing %.3f s, ordering and formatting %.3f s, writing %.3f s; "
                    "%u rounds, %llu records refined\n",
                    res.shape == HPN_KSEQ_FASTA ? "fasta" : res.shape == HPN_KSEQ_FASTQ ? "fastq" : "none", (unsigned long long)res.n_records,
                    (double)(fed - begin) / 1e6, (double)(ordered - fed) / 1e6, (double)(usec() - ordered) / 1e6, res.rounds,
                    (unsigned long long)res.refined);
        quick_exit_ok();
    }
    if (!is_stdin) slurp_or_refuse(tool, path, mem);
    if (memchr(mem.data(), 0, mem.size())) refuse(tool, path, "NUL byte in the text");
    const KseqAnswer a = kseq_map(mem.data(), mem.size());
    if (btree && !a.one_length) kseq_mixed_lengths(tool, path, a.first_len, a.other_len);
    fprintf(stderr, "%llu\n", (unsigned long long)a.n_distinct);
    const long long ordered = usec();
    if (!a.out.empty() && fwrite(a.out.data(), 1, a.out.size(), stdout) != a.out.size()) {
        fprintf(stderr, "%s: writing standard output failed (%s)\n", tool, strerror(errno));
        leave(2);
    }
    fflush(stdout);
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] kseq: route host, %llu records; reading %.3f s, parsing and ordering %.3f s, writing %.3f s\n",
                (unsigned long long)a.n_records, (double)(fed - begin) / 1e6, (double)(ordered - fed) / 1e6, (double)(usec() - ordered) / 1e6);
    quick_exit_ok();
}

}  // namespace hpn
