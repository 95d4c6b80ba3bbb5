// bam_view.hpp -- what kernels/bam_view.hip and the session over it (hpn_bamview.hip) share: the rules, the reasons, the launchers.
#pragma once
#include "bam_sort.hpp"

namespace hpn {

// why a record is not the device's (include/hpngs.h names them): a float aux field (no %g here); an A field of value 0; a name
// whose first NUL is not its last byte; an unknown aux type or a B array of negative length; a name, CIGAR, sequence, quality or
// aux field that does not end inside the record; pos or mpos of 2^31 - 1; the 2^31-th record; a refID or mate refID the header
// lacks; a CIGAR op above 9 (BAM_CIGAR_STR ends there)
enum { kVwrFloat = 1, kVwrANul = 2, kVwrName = 3, kVwrAuxType = 4, kVwrLayout = 5, kVwrPos = 6, kVwrRecords = 7, kVwrTarget = 8, kVwrCigarOp = 9 };
constexpr int kVwReasonBits = 4;       // word kInfoBad: ordinal << 4 | reason

enum { kVwBam = 0, kVwText = 1, kVwCount = 2 };        // what the session emits
enum { kVwDec = 0, kVwHex = 1, kVwStr = 2 };           // the flag's style in text

constexpr int kVwThreads = 256;

struct VwRules {
    uint32_t flag_on, flag_off, min_mapq;
    int32_t min_qlen, qual_scale;
    uint32_t subsample, seed, threshold;   // drop where ((X31(name) + seed) & 0xffffff) >= threshold
    uint32_t emit, flag_style;
    uint32_t n_targets;
    const uint8_t *names;                  // the targets' names behind one another
    const uint32_t *name_off;              // n_targets + 1 offsets into them
    // the read-group rule: the IDs behind one another -- [0, n_r) the one of -r, [n_r, n_r + n_R) the set of -R, the n_l behind
    // them the IDs whose LB is the library -- and n_r + n_R + n_l + 1 offsets into them; rg_rule: kVwRuleId | kVwRuleSet | kVwRuleLib
    uint32_t rg_rule, n_r, n_R, n_l;
    const uint8_t *ids;
    const uint32_t *id_off;
};
enum { kVwRuleId = 1, kVwRuleSet = 2, kVwRuleLib = 4 };

// per record of the batch, in place: size[], soff[], keep[], llen[] (text sessions: the line's bytes with its newline), info words
hipError_t launch_bamview_classify(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, VwRules r, uint32_t *size,
                                   u64 *soff, uint32_t *keep, uint32_t *llen, u64 *info, hipStream_t st);
// order[kidx[i]] = i for every kept record i (kidx: the exclusive scan of keep)
hipError_t launch_bamview_compact(const uint32_t *keep, const uint32_t *kidx, uint64_t n, uint32_t *order, hipStream_t st);
// klen[j] = llen[order[j]], 64 bits wide for the scan that places the lines
hipError_t launch_bamview_klen(const uint32_t *llen, const uint32_t *order, uint64_t n_out, u64 *klen, hipStream_t st);
// output records [first, first + cnt) as SAM lines at text + (toff[first + k] - toff[first]); 16 lanes a record
hipError_t launch_bamview_format(const uint8_t *store, const u64 *soff, const uint32_t *size, const uint32_t *order, const u64 *toff, uint64_t first,
                                 uint64_t cnt, VwRules r, uint8_t *text, hipStream_t st);
// the slice's gathered records: every quality byte q becomes min(q * scale, 93); 16 lanes a record
hipError_t launch_bamview_qscale(const u64 *out_off, uint64_t first, uint64_t cnt, int32_t scale, uint8_t *pay, hipStream_t st);

}  // namespace hpn
