// A stand-alone program around highperformancengs_amd/csrc/host/bam_rmdup_host.hpp for tests/test_rmdup_golden.py, which builds
// it twice -- plain and with -fsanitize=address,undefined -- and runs it as a process of its own: `samtools rmdup` on the CPU, the
// route bin/bam_rmdup takes with -s, -S or HPN_BAM_GPU=0 and falls back to.  argv: samtools rmdup's own; with fewer than two
// arguments behind the options the reference's usage text and status 1.
#include "host/bam_rmdup_host.hpp"

int main(int argc, char *argv[])
{
    hpn::rmdup::Options o;
    if (!hpn::rmdup::parse_args(argc, argv, o)) return 1;
    return hpn::rmdup::rmdup_on_host(o);
}
