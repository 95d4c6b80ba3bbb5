// map_kseq -- drop-in for the reference tool of the same name (map_kseq.cpp): the first record of every distinct sequence of a
// FASTA / FASTQ file, in std::map<std::string>'s order of the sequences; framing, ordering and formatting run on MI355X through
// libhpngs (host/kseq_tool.hpp).
//
//   map_kseq <file>      "-" or an empty name: standard input; plain and gzip alike; a missing file is made, as there
#include "../host/kseq_tool.hpp"

int main(int argc, char *argv[]) { return hpn::kseq_tool_main(argc, argv, "map_kseq", false); }
