// pair_cmp.hpp -- what one lane of kernels/fastq_pair.hip does with a name: the offset of its first space (k_pair_klen) and its
// 16 bytes of pick_pair.c's strncmp(a.name, b.name, strchr(a.name, ' ') - a.name).  Plain C++ that a host compiler takes as
// well: the bodies are run on the host against a byte loop (docs/kernels/fastq_pair.md).
//
// The reference compares unsigned bytes up to the first difference, a NUL in both, or k bytes.  The names here hold no NUL byte
// (the framer refuses such text), b's name ends in one, and a name without a space has k = (size_t)(NULL - name): the whole
// name and its NUL are compared.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPN_PAIR_FN __host__ __device__ __forceinline__
#else
#define HPN_PAIR_FN inline
#endif

namespace hpn {

constexpr uint32_t kPairNoSpace = 0xffffffffu;   // k of a name without a space
constexpr uint32_t kPairNone = 0xffffffffu;      // no differing byte; no mate
constexpr int kPairTeam = 4;                     // lanes per record: 64 bytes of both names per step

// The offset of the first ' ' in name[0, nlen), or kPairNoSpace.  16-byte loads; the last one is moved back so that it ends
// with the name, a name shorter than 16 bytes is read by bytes: no load reaches behind the name's last byte.
HPN_PAIR_FN uint32_t pair_klen(const uint8_t *name, uint32_t nlen)
{
    if (nlen < 16u) {
        for (uint32_t b = 0; b < nlen; ++b)
            if (name[b] == ' ') return b;
        return kPairNoSpace;
    }
    for (uint32_t o = 0; o < nlen; o += 16u) {
        const uint32_t at = o + 16u <= nlen ? o : nlen - 16u;   // (the bytes in front of o hold no space: the first hit is the first space)
        uint64_t v[2];
        __builtin_memcpy(v, name + at, 16);
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint64_t x = v[h] ^ 0x2020202020202020ull;
            const uint64_t z = (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;   // its lowest set bit marks the first zero byte
            if (z) return at + 8u * h + ((uint32_t)__builtin_ctzll(z) >> 3);
        }
    }
    return kPairNoSpace;
}

// strncmp(a, b, k) over names of nal and nbl bytes: *len bytes of both are compared, and *tail is the result when they agree.
HPN_PAIR_FN void pair_span(uint32_t k, uint32_t nal, uint32_t nbl, uint32_t *len, int *tail)
{
    const uint32_t K = k == kPairNoSpace ? nal + 1u : k;   // without a space a's NUL takes part
    const uint32_t m = nal < nbl ? nal : nbl;
    if (K <= m) *len = K, *tail = 0;
    else *len = m, *tail = nal == nbl ? 0 : (nal < nbl ? -1 : 1);   // the shorter name's NUL against a byte that is none
}

// One lane's piece: the 16 bytes of a[0, len) and b[0, len) from o on (the last piece moved back so that it ends at len; fewer
// than 16 bytes in all: lane 0 reads them one by one).  Returns the position of the first differing byte it saw, or kPairNone,
// and *less: a's byte is the smaller one.
HPN_PAIR_FN uint32_t pair_lane_diff(const uint8_t *a, const uint8_t *b, uint32_t len, uint32_t o, bool *less)
{
    *less = false;
    if (o >= len) return kPairNone;
    if (len < 16u) {   // (o is 0)
        for (uint32_t p = 0; p < len; ++p)
            if (a[p] != b[p]) {
                *less = a[p] < b[p];
                return p;
            }
        return kPairNone;
    }
    const uint32_t at = o + 16u <= len ? o : len - 16u;
    uint64_t x[2], y[2];
    __builtin_memcpy(x, a + at, 16);
    __builtin_memcpy(y, b + at, 16);
    for (uint32_t h = 0; h < 2u; ++h) {
        const uint64_t d = x[h] ^ y[h];
        if (d) {
            const uint32_t s = (uint32_t)__builtin_ctzll(d) & ~7u;   // little-endian: the first byte is the lowest
            *less = ((x[h] >> s) & 0xffu) < ((y[h] >> s) & 0xffu);
            return at + 8u * h + (s >> 3);
        }
    }
    return kPairNone;
}

}  // namespace hpn
