// check_block.h -- the arithmetic of the text digest (./harc -c -V; README: "-V and what it promises"), once for host and device, and the record read.check.
//   T(text) = (bytes, newlines, D),  D = sum over the bytes of mix64(((o + 1) << 8) | byte_o) mod 2^64, o the byte's offset in the whole text.
// The key is injective for o < 2^56 and mix64 (devutil.h's finaliser, restated here for host code that includes no device header) is a bijection of the 64-bit
// words: one changed byte always changes D.  A sum: pieces that know their first offset add up to the digest of the whole, in any order.  Not cryptographic.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define CK_HD __host__ __device__ __forceinline__
#else
#define CK_HD static inline
#endif

CK_HD uint64_t ck_mix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
// the term of the byte at offset `pos` of the whole text
CK_HD uint64_t ck_term(uint64_t pos, uint32_t byte) { return ck_mix64(((pos + 1) << 8) | (uint64_t)(byte & 0xFFu)); }
// the eight bytes of the little-endian word w that the bits of `keep` name (bit k: byte k), byte k at offset pos + k: their terms are added to *d, their newlines to *nl
CK_HD void ck_word(uint64_t w, uint32_t keep, uint64_t pos, uint64_t *d, uint32_t *nl)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const uint32_t b = (uint32_t)(w >> (8 * k)) & 0xFFu;
        const bool in = (keep >> k) & 1u;
        *d += in ? ck_term(pos + (uint64_t)k, b) : 0;
        *nl += (in && b == 10u) ? 1u : 0u;
    }
}
// a piece in host memory, serially: acc[0] += n, acc[1] += newlines, acc[2] += D terms
static inline void ck_digest_host(const uint8_t *p, uint64_t n, uint64_t first, uint64_t acc[3])
{
    uint64_t d = 0, nl = 0;
    for (uint64_t i = 0; i < n; i++) { d += ck_term(first + i, p[i]); nl += p[i] == 10; }
    acc[0] += n; acc[1] += nl; acc[2] += d;
}

// ---- read.check: "HARCV1", then one item per line, values as 16 lowercase hex digits
//   reads <count> <sum> <xor>   order <bytes> <D>   ids <bytes> <lines> <D>   quality <bytes> <lines> <D>
#define CK_MAGIC "HARCV1"
static inline int ck_format_reads(char *out, size_t cap, const uint64_t sig[3])
{
    return snprintf(out, cap, "reads %016llx %016llx %016llx\n", (unsigned long long)sig[0], (unsigned long long)sig[1], (unsigned long long)sig[2]);
}
static inline int ck_format_order(char *out, size_t cap, const uint64_t t[3])
{
    return snprintf(out, cap, "order %016llx %016llx\n", (unsigned long long)t[0], (unsigned long long)t[2]);
}
