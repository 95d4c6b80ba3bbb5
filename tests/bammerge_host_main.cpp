// A stand-alone program around highperformancengs_amd/csrc/host/bam_merge_host.hpp for tests/test_bammerge_golden.py, which builds
// it twice -- plain and with -fsanitize=address,undefined -- and runs it as a process of its own: `samtools merge` on the CPU, the
// route bin/bam_merge takes with -n, -r or HPN_BAM_GPU=0 and falls back to.  argv: samtools merge's own; with fewer than three
// file arguments behind the options the reference's usage text and status 1.
#include "host/bam_merge_host.hpp"

int main(int argc, char *argv[])
{
    hpn::bammerge::Options o;
    const int early = hpn::bammerge::parse_args(argc, argv, o);
    return early ? early : hpn::bammerge::merge_on_host(o);
}
