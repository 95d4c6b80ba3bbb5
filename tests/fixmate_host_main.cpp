// A stand-alone program around highperformancengs_amd/csrc/host/bam_fixmate_host.hpp for tests/test_fixmate_golden.py, which builds
// it twice -- plain and with -fsanitize=address,undefined -- and runs it as a process of its own: `samtools fixmate` on the CPU, the
// route bin/bam_fixmate takes with HPN_BAM_GPU=0, from or to a pipe, and falls back to.  argv: samtools fixmate's own; with fewer
// than two file arguments behind the options the reference's usage text and status 1.
#include "host/bam_fixmate_host.hpp"

int main(int argc, char *argv[])
{
    hpn::fixmate::Options o;
    if (!hpn::fixmate::parse_args(argc, argv, o)) return 1;
    return hpn::fixmate::fixmate_on_host(o);
}
