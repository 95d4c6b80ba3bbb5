// hpn_sorter.hpp -- the refinement sort of hpn_sort.hip as hpn_fastq_sort_* and hpn_kseq_* hold it: its arrays, its key mode and an
// info block of its own (the words of kSiBits lie in no session's block).
#pragma once
#include "hpn_store.hpp"

namespace hpn {

struct SorterArrays {   // what a new session must not inherit
    Scratch order, key, val, key_tmp, val_tmp, hist, offs, status, word1, val1, word, head, gid, stay, keep, at;
    Scratch t_pos[2], t_ord[2], t_len[2], t_run[2], t_kp[2];
};

struct Sorter : SorterArrays {
    InfoBlock info;
    int by_name = 0, bytes_only = 0;   // bytes_only: the third key mode (hpn_kseq_*), the sequence without its length in front
    void drop() { static_cast<SorterArrays &>(*this) = SorterArrays(); }
};

// hpn_sort.hip: the n records that `desc` describes in `text`, by the sorter's key mode, into u->order; res->rounds and
// res->refined say what it took
int order_records(hpn_ctx *c, Sorter *u, const uint8_t *text, const void *desc, uint32_t n, hpn_sort_result *res);

}  // namespace hpn
