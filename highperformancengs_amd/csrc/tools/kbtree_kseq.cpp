// kbtree_kseq -- drop-in for the reference tool of the same name (kbtree_kseq.c) where that has an answer: with sequences of ONE
// length its B-tree is a set in strcmp order and it prints what map_kseq prints, byte for byte.  With more than one length its
// comparison -- "length, then strcmp" as an unparenthesised ?: inside kbtree.h's __cmp(x, y) < 0 -- is true both ways and what the
// tree holds is an artefact of its shape: this tool names the first two lengths and leaves with status 2 (host/kseq_tool.hpp).
//
//   kbtree_kseq <file>   "-" or an empty name: standard input; plain and gzip alike; a missing file is made, as there
#include "../host/kseq_tool.hpp"

int main(int argc, char *argv[]) { return hpn::kseq_tool_main(argc, argv, "kbtree_kseq", true); }
