// linesel.h -- where line k of a text of variable-length lines starts (./harc -d -r; README: "-r and what it promises"), the arithmetic once for host and device.
// A text of n bytes holds as many lines as newlines; line k (counted from 0) starts at byte 0 for k = 0, else one past the k-th newline -- n itself when that
// newline is the last byte -- and nowhere (LS_NONE) when the text holds fewer than k newlines.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LS_HD __host__ __device__ __forceinline__
#else
#define LS_HD static inline
#endif

#define LS_NONE 0xFFFFFFFFFFFFFFFFull

// bit j of the result: byte j of the little-endian word w is a newline.  Exact: no borrow runs from one byte into the next
LS_HD uint32_t ls_newline_bits(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte of x that is zero
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
// the bytes of the 16-byte chunk that starts `a` bytes into the hull [mis, hull) of a text: bit j = byte j belongs to the text
LS_HD uint32_t ls_keep_bits(uint64_t a, uint64_t mis, uint64_t hull)
{
    uint32_t keep = 0xFFFFu;
    if (a < mis) keep &= 0xFFFFu << (uint32_t)(mis - a);
    if (a + 16 > hull) keep &= 0xFFFFu >> (uint32_t)(a + 16 - hull);
    return keep;
}
// where the r-th set bit of m is (r counted from 1, m holds at least r bits)
LS_HD uint32_t ls_nth_bit(uint32_t m, uint32_t r)
{
    for (uint32_t i = 1; i < r; i++) m &= m - 1u;
    uint32_t j = 0;
    while (!((m >> j) & 1u)) j++;
    return j;
}

// ---- the host twin: out[0] = the newlines of the text, out[1] = where line k starts
static inline void ls_line_offset_host(const uint8_t *t, uint64_t n, uint64_t k, uint64_t out[2])
{
    uint64_t nl = 0, at = k == 0 ? 0 : LS_NONE, i = 0;
    while (i < n) {
        const uint8_t *e = (const uint8_t *)memchr(t + i, '\n', (size_t)(n - i));
        if (!e) break;
        nl++;
        i = (uint64_t)(e - t) + 1;
        if (nl == k) at = i;
    }
    out[0] = nl; out[1] = at;
}
