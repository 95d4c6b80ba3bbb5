// twoBit2seq -- drop-in for the reference tool of the same name (twoBit2seq.c): what fastq2twobit packed, as one sequence per
// line; the unpacking runs on MI355X through libhpngs, chunk by chunk, so the file may be larger than the device's memory.
//
//   twoBit2seq [-i FILE] [-o PREFIX] [-c N] [-h]
//
//   -i        default "-": standard input (plain bytes: the reference reads with fread, not through zlib).
//   -o        PREFIX.decompress, default "out"; a prefix that begins with '-' means standard output.   -c N  parsed and ignored.
//   input     two header bytes, seqlen and packedLen, then records of packedLen bytes; a trailing partial record is dropped.
//   output    per record seqlen characters (0 'T', 1 'C', 2 'A', 3 'G', the first base in a byte's top bits) and '\n'.  The
//             reference unpacks from a zeroed buffer: with packedLen < (seqlen + 3) >> 2 the missing bases are 'T', a larger
//             packedLen skips the surplus bytes.  Fewer than two bytes of input: an empty output.
//   stderr    the reference's line, "done read file at T s".
//
// Where the reference has no answer -- packedLen == 0 in an input of two or more bytes: its fread of 0 bytes never meets the
// end of the file and it prints newlines for ever -- this tool says so and leaves with status 2 before it makes the output.
#include <errno.h>
#include <getopt.h>

#include <vector>

#include "../host/report.hpp"
#include "../host/text_stream.hpp"

using namespace hpn;

static void usage(const char *prog)
{
    fprintf(stderr,
            "\nUsage: %s [-i Infile] [-o OUTFILE] [-c compress_level] [-h]\n"
            "  Unpacks the 2-bit file that fastq2twobit wrote into one ATCG sequence per line (MI355X build of\n"
            "  HighPerformanceNGS twoBit2seq).\n"
            "Example1:\n  %s -i reads_sort_by_seq.fq -o reads\n\n"
            "   [-i Infile] = Infile, default standard input.                    [option]\n"
            "   [-o OUTPUT] = prefix of OUTPUT.decompress, default 'out'; a\n"
            "                 leading '-' means standard output.                 [option]\n"
            "   [-c level]  = accepted and ignored, as in the reference.         [option]\n"
            "   [-h] This helpful help screen.                                   [option]\n\n",
            prog, prog);
    exit(1);
}

// up to n bytes, short only at the end of the input
static size_t read_full(int fd, uint8_t *dst, size_t n)
{
    size_t got = 0;
    while (got < n) {
        const ssize_t k = read(fd, dst + got, n - got);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) break;
        got += (size_t)k;
    }
    return got;
}

int main(int argc, char *argv[])
{
    bind_before_runtime();
    const char *infile = "-", *outfile = "out";
    if (argc < 2) usage(argv[0]);
    int opt;
    while ((opt = getopt(argc, argv, "i:o:c:h?")) != -1) {
        switch (opt) {
        case 'i': infile = optarg; break;
        case 'o': outfile = optarg; break;
        case 'c': (void)atoi(optarg); break;
        case '?':
        case 'h': usage(argv[0]); break;
        default: fprintf(stderr, "error parameter!\n"); break;
        }
    }
    // fopen_input_stream (IO_stream.h:53-67): a missing file is created empty
    int fd = STDIN_FILENO;
    if (!(strncmp(infile, "-", 1) == 0 || !strcmp(infile, ""))) {
        fd = open(infile, O_CREAT | O_RDONLY, 0666);
        if (fd == -1) {
            fprintf(stderr, "Failed to create input file (%s)", infile);
            leave(2);
        }
    }
    const long long begin = usec();
    uint8_t header[2] = {0, 0};
    const size_t have = read_full(fd, header, 2);
    const uint32_t seqlen = header[0], plen = header[1];
    if (have == 2 && plen == 0) {
        fprintf(stderr, "twoBit2seq: %s: packedLen is 0 (the reference has no answer there: it never meets the end of the file)\n", infile);
        leave(2);
    }
    FILE *out = fcreat_outfile(outfile, ".decompress");
    if (!out) leave(2);
    double t_read = 0, t_dev = 0, t_write = 0;
    uint64_t records = 0;
    if (have == 2) {
        hpn_ctx *ctx = open_tool_ctx();
        // a chunk: a whole number of records, about text_chunk_bytes() of input and at most four times that of output
        const uint64_t budget = text_chunk_bytes();
        uint64_t per = budget / plen;
        if (per > 4 * budget / (seqlen + 1u)) per = 4 * budget / (seqlen + 1u);
        if (per < 1) per = 1;
        std::vector<uint8_t> in_buf(per * plen), out_buf(per * (seqlen + 1u));
        for (;;) {
            long long t0 = usec();
            const size_t got = read_full(fd, in_buf.data(), in_buf.size());
            const uint64_t n = got / plen;   // (a partial record can only be the input's last bytes: dropped)
            long long t1 = usec();
            t_read += (double)(t1 - t0) / 1e6;
            if (n) {
                uint64_t bytes = 0;
                const int rc = hpn_twobit_unpack(ctx, seqlen, plen, in_buf.data(), n, out_buf.data(), out_buf.size(), &bytes);
                if (rc != HPN_OK) die_hpn(ctx, rc, "hpn_twobit_unpack");
                t0 = usec();
                t_dev += (double)(t0 - t1) / 1e6;
                if (fwrite(out_buf.data(), 1, bytes, out) != bytes) {
                    fprintf(stderr, "twoBit2seq: writing %s.decompress failed (%s)\n", outfile, strerror(errno));
                    leave(2);
                }
                t_write += (double)(usec() - t0) / 1e6;
                records += n;
            }
            if (got < in_buf.size()) break;
        }
    }
    fprintf(stderr, "done read file at %.3f s\n", (double)(usec() - begin) / CLOCKS_PER_SEC);
    if (fclose(out) != 0) {
        fprintf(stderr, "twoBit2seq: writing %s.decompress failed (%s)\n", outfile, strerror(errno));
        leave(2);
    }
    if (getenv("HPN_TIMING"))
        fprintf(stderr, "[hpn] twobit unpack: reading %.3f s, unpacking (with both copies) %.3f s, writing %.3f s; %llu records\n", t_read, t_dev, t_write,
                (unsigned long long)records);
    quick_exit_ok();
}
