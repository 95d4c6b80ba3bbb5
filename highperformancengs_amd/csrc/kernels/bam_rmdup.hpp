// bam_rmdup.hpp -- what kernels/bam_rmdup.hip and its session (hpn_rmdup.hip) share: the arrays, the info words, the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpn {
typedef unsigned long long u64;

// info (u64 words, kept on the device from _begin to _finish):
//   [0] lowest (ordinal << 4 | reason), ~0 none      [1] stream offset of the batch's first record   [2] ... behind its last
enum { kRmBad = 0, kRmFirst, kRmEnd, kRmWords = 8 };
enum { kRmPass = 0, kRmHead = 1, kRmTail = 2, kRmUnplaced = 3 };
enum { kEvNone = 0, kEvIns = 1, kEvTail = 2 };
// reasons (include/hpngs.h: HPN_RMDUP_*)
enum { kRsTidBack = 1, kRsPosBack, kRsRecords, kRsRgType, kRsAux, kRsName, kRsInconsistent, kRsCollision, kRsFirstUnplaced, kRsTidBeyond, kRsPosNeg, kRsFields };

struct RmArrays {          // one entry per input record, by ordinal
    u64 *tp;               // (uint32_t)refID << 32 | (uint32_t)pos; unplaced: 0xffffffff << 32
    uint32_t *cls, *isize, *qsum, *lib, *size;
    u64 *hash, *soff;
};

struct RmIds {             // the header's ID -> library table: ID k is bytes[off[k] .. off[k + 1]), its library lib[k]; library 0: none
    const uint8_t *bytes;
    const uint32_t *off, *lib;
    uint32_t n;
};

struct RmWork {            // what _finish makes, by ordinal unless said otherwise
    uint32_t *rb, *hf;     // run boundary, head flag (scanned into rsc, hsc: n + 1 entries)
    uint32_t *rsc, *hsc, *rid, *runstart;      // runstart: by run ordinal, n_runs + 1 entries
    uint32_t *evkind, *evrec, *slot, *drop;    // the event at the time of this record: kind, whose name; slot: survivor + 1 where a group begins here
    uint32_t *now, *sl, *cnow, *cslot;         // flags and their scans
};

hipError_t launch_rmdup_classify(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t base, uint64_t store_at, uint32_t n_ref, const RmArrays &A,
                                 const RmIds &ids, u64 *info, hipStream_t st);
hipError_t launch_rmdup_runs(const RmArrays &A, const RmWork &W, uint64_t n, uint32_t n_ref, uint32_t *present, hipStream_t st);
hipError_t launch_rmdup_scatter(const RmArrays &A, const RmWork &W, uint64_t n, u64 *hkey, uint32_t *hval, hipStream_t st);
hipError_t launch_rmdup_runkey(const RmWork &W, uint64_t m, u64 *hkey, const uint32_t *hval, hipStream_t st);
hipError_t launch_rmdup_groups(const RmArrays &A, const RmWork &W, uint64_t m, const uint32_t *hval, u64 *libs, hipStream_t st);
hipError_t launch_rmdup_evkey(const RmArrays &A, const RmWork &W, uint64_t n, u64 *ekey, uint32_t *eval, hipStream_t st);
hipError_t launch_rmdup_names(const uint8_t *store, const RmArrays &A, const RmWork &W, uint64_t n, const u64 *ekey, const uint32_t *eval, u64 *unmatched,
                              u64 *info, hipStream_t st);
hipError_t launch_rmdup_flags(const RmArrays &A, const RmWork &W, uint64_t n, hipStream_t st);
hipError_t launch_rmdup_place(const RmWork &W, uint64_t n, uint64_t n_out, uint32_t *order, hipStream_t st);

}  // namespace hpn
