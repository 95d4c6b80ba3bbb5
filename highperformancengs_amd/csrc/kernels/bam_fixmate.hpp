// bam_fixmate.hpp -- what kernels/bam_fixmate.hip and the session over it (hpn_bamfixmate.hip) share: the info words behind
// bam_sort.hpp's, the classes, roles and reasons, the arrays, the launchers.
#pragma once
#include "bam_sort.hpp"

namespace hpn {

// info words [0..2] as bam_sort.hpp names them (k_fix_classify fills what k_sort_keys fills); [9..12] k_fix_plan's counts:
// pairs, singletons (the final pending record is none), CT tags, bytes the CT tags add
enum { kFxPairs = 9, kFxSingles, kFxTags, kFxAdded };

enum { kFxLive = 0, kFxSkipTid = 1, kFxSkipSecondary = 2 };      // meta & 3; meta >> 16: the flag behind the 0x4 update
enum { kFxFirst = 0, kFxSecond, kFxSingle, kFxPending, kFxSkipped };
// why a record is not the device's: a CIGAR op above 8; a name whose first NUL is not its last byte (or no name at all); a refID
// the header does not have; a name and CIGAR that do not fit into the record; the 2^31-th record (the session's cap)
enum { kFxrCigarOp = 1, kFxrName = 2, kFxrTarget = 3, kFxrLayout = 4, kFxrRecords = 5 };

constexpr int kFxThreads = 256;

struct FxRecords {      // by ordinal, filled batch by batch
    const uint8_t *store;
    const u64 *soff;
    const uint32_t *size;
    uint32_t *meta;     // class | flag << 16
    int32_t *cend;      // bam_calend
    uint32_t *clen;     // the CIGAR's text: decimal digits + one letter per op
};

struct FxPatch {        // by ordinal, made by _finish: what the output record differs in from the stored one
    uint32_t *flag, *mtid, *mpos, *isize;
    uint32_t *extra;    // bytes of the CT field (0: none)
    uint32_t *partner;  // the CT carrier's mate (the upper record of the text)
};

hipError_t launch_bamfix_classify(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, uint32_t n_targets,
                                  const uint32_t *target_len, uint32_t *size, u64 *soff, uint32_t *meta, int32_t *cend, uint32_t *clen, u64 *info,
                                  hipStream_t st);
// live[i] = 1 for a live record (the input of the scan that numbers them)
hipError_t launch_bamfix_live(const uint32_t *meta, uint64_t n, uint32_t *live, hipStream_t st);
// liveidx[lidx[i]] = i for every live record i
hipError_t launch_bamfix_compact(const uint32_t *meta, const uint32_t *lidx, uint64_t n, uint32_t *liveidx, hipStream_t st);
// head[l] = 1 where live record l's name differs from live record l - 1's (and for l = 0)
hipError_t launch_bamfix_heads(FxRecords r, const uint32_t *liveidx, uint64_t n_live, uint32_t *head, hipStream_t st);
// runstart[run] = the live ordinal of the run's first record (rid: the exclusive scan of head)
hipError_t launch_bamfix_runstart(const uint32_t *head, const uint32_t *rid, uint64_t n_live, uint32_t *runstart, hipStream_t st);
// role[i] and writes[i]: how many records the reference writes while record i is the current one
hipError_t launch_bamfix_roles(const uint32_t *meta, const uint32_t *lidx, uint64_t n, uint64_t n_live, const uint32_t *head, const uint32_t *rid,
                               const uint32_t *runstart, int remove_reads, uint32_t *role, uint32_t *writes, hipStream_t st);
// order[slot of i] = i, the patch of every record, the counts (woff: the exclusive scan of writes, n + 1 entries)
hipError_t launch_bamfix_plan(FxRecords r, const uint32_t *lidx, const uint32_t *liveidx, uint64_t n, const uint32_t *role, const uint32_t *writes,
                              const uint32_t *woff, uint32_t *order, FxPatch p, u64 *info, hipStream_t st);
// the slice's gathered records [first, first + cnt) at pay: the five core fields rewritten, the CT field behind the carriers
hipError_t launch_bamfix_apply(FxRecords r, FxPatch p, const uint32_t *order, const u64 *out_off, uint64_t first, uint64_t cnt, uint8_t *pay,
                               hipStream_t st);

}  // namespace hpn
