// A stand-alone program around highperformancengs_amd/csrc/host/bam_view_host.hpp for tests/test_view_golden.py, which builds it
// twice -- plain and with -fsanitize=address,undefined -- and runs it as a process of its own: `samtools view` on the CPU, the
// route bin/bam_view takes with HPN_BAM_GPU=0, from a pipe, with BAM to stdout, and falls back to.  argv: samtools view's own.
#include "host/bam_view_host.hpp"

int main(int argc, char *argv[])
{
    hpn::view::Options o;
    const int early = hpn::view::parse_args(argc, argv, o);
    if (early) return early;
    return hpn::view::view_on_host(o);
}
