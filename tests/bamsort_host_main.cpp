// A stand-alone program around highperformancengs_amd/csrc/host/bam_sort_host.hpp for tests/test_bamsort_golden.py, which builds
// it twice -- plain and with -fsanitize=address,undefined -- and runs it as a process of its own: `samtools sort` on the CPU, the
// route bin/bam_sort takes with -n or HPN_BAM_GPU=0 and falls back to.  argv: samtools sort's own; with fewer than two
// arguments behind the options the reference's usage text and status 1.
#include "host/bam_sort_host.hpp"

int main(int argc, char *argv[])
{
    hpn::bamsort::Options o;
    if (!hpn::bamsort::parse_args(argc, argv, o)) return 1;
    return hpn::bamsort::sort_on_host(o);
}
