// sv_block.h -- one block of the packed stream file X.hs (README: "The packed stream file"): m bytes of any values -> u32 payload_bytes and the payload, stored
// (mode 0), coded with one static table (mode 1, order 0) or with a table per previous byte (mode 2, order 1), rANS in 256 strands.  Every function that
// decides a byte of a block lives here once: spack.hip runs them on the device (a workgroup per block, a lane per strand), harc_amd_spack_host /
// harc_amd_sunpack_host run them in a row on the host, and tests/test_spack_host.py builds this file with g++ and sanitizers as a stand-alone program.  No local
// arrays: on the device they would live in private memory.  The coder step, the decoder step and the little-endian helpers are qv_block.h's, the row
// normaliser is id_block.h's (rows here have 256 symbols, as its difference and number rows have), the CRC-32 is that of the BGZF code.
//
// Strands.  q = ceil(m / 256); strand s holds the bytes [min(m, s q), min(m, (s + 1) q)) of the block and is coded on its own: the context of its first byte is 0.
//
// Tables.  A row is 256 u32, one per byte value: first the count, then frequency | cumulative << 16 (id_norm_counts).  Mode 1 has one row, mode 2 a row per
// previous byte at tab[previous << 8 | byte].  In the file a row is 32 bytes of bitmap (bit y of the 256-bit little-endian number: byte y >> 3, bit y & 7) and
// the u16 frequencies of the symbols whose bit is set, each >= 1, summing to 4096.
//
// The mode.  The encoder codes every strand both ways, sums the exact sizes and takes the smallest payload (sv_choose): stored wins ties, then mode 1.
#pragma once
#include <stdint.h>
#include "id_block.h"
#include "deflate_member.h"

enum {
    SV_OK = 0,
    SV_E_MODE = 1,         // the mode byte is above 2
    SV_E_SIZE = 2,         // block_text_bytes is not the block's share of the text; a stored payload that is not 9 + text bytes; a coded one shorter than its head
    SV_E_BITMAP = 3,       // a bitmap without a bit
    SV_E_ROW = 4,          // a present symbol without a frequency, or a row that does not sum to 4096
    SV_E_LENGTHS = 5,      // the strand coded bytes do not sum to the rest of the payload
    SV_E_SHORT = 6,        // a strand with text of fewer than 4 coded bytes; a strand without text that is not empty
    SV_E_TRUNC = 7,        // the decoder needs a byte behind the strand's end                                  (= QV_E_TRUNC)
    SV_E_CONTEXT = 8,      // a slot that belongs to no symbol of the row, or a row that is absent              (= QV_E_CONTEXT)
    SV_E_END = 9,          // the state is not 2^23 or the strand has bytes left after its last byte (or its first state is below 2^23)
    SV_E_CRC = 10,         // the CRC-32 of the text is not the one in the payload
};

#define SV_STRANDS 256u
#define SV_FILE_HEADER 32u
#define SV_DEFAULT_B (1u << 22)
#define SV_MAX_B (1u << 30)
#define SV_HEAD0 9u                                    // mode, block_text_bytes, crc32
#define SV_TAB0 (SV_HEAD0 + 32u)                       // ... the first bitmap
#define SV_LENS (4u * SV_STRANDS)
#define SV_HEAD1_MAX (SV_TAB0 + 512u + SV_LENS)
#define SV_HEAD2_MAX (SV_TAB0 + 256u * (32u + 512u) + SV_LENS)
#define SV_PREFIX (4u + SV_HEAD0)
#define SV_E_NONE 0xFFFFFFFFu

QV_HD uint64_t sv_blocks(uint64_t n, uint32_t B) { return B ? (n + B - 1) / B : 0; }
QV_HD uint64_t sv_bound(uint64_t n, uint32_t B) { return SV_FILE_HEADER + n + (uint64_t)SV_PREFIX * sv_blocks(n, B); }
QV_HD uint32_t sv_block_text(uint64_t n, uint32_t B, uint64_t b) { const uint64_t rest = n - b * B; return rest < B ? (uint32_t)rest : B; }
QV_HD uint32_t sv_strand_q(uint32_t m) { return (m + SV_STRANDS - 1u) / SV_STRANDS; }
QV_HD uint32_t sv_strand_at(uint32_t m, uint32_t s) { const uint64_t a = (uint64_t)s * sv_strand_q(m); return a < m ? (uint32_t)a : m; }
QV_HD uint32_t sv_strand_bytes(uint32_t m, uint32_t s) { return sv_strand_at(m, s + 1u) - sv_strand_at(m, s); }
QV_HD uint32_t sv_slab_bytes(uint32_t m) { return qv_slab_bytes(sv_strand_q(m)); }                     // scratch of one strand coded one way
QV_HD void sv_file_header(uint8_t *h, uint32_t B, uint64_t n)
{
    h[0] = 'H'; h[1] = 'A'; h[2] = 'R'; h[3] = 'C'; h[4] = 'S'; h[5] = '1'; h[6] = 0; h[7] = 0;
    qv_put32(h + 8, n ? B : 0u); qv_put32(h + 12, 0); qv_put64(h + 16, n); qv_put64(h + 24, 0);
}
QV_HD int sv_magic_ok(const uint8_t *h) { return h[0] == 'H' && h[1] == 'A' && h[2] == 'R' && h[3] == 'C' && h[4] == 'S' && h[5] == '1' && h[6] == 0 && h[7] == 0; }
QV_HD uint32_t sv_code(int e) { return e ? (uint32_t)e : SV_E_NONE; }
// stored wins ties, then mode 1.  p1, p2: the payload bytes of the two coded modes
QV_HD uint32_t sv_choose(uint32_t m, uint64_t p1, uint64_t p2)
{
    const uint64_t p0 = (uint64_t)SV_HEAD0 + m;
    if (p0 <= p1 && p0 <= p2) return 0u;
    return p1 <= p2 ? 1u : 2u;
}

// ---------------------------------------------------------------------------------------------------------------- a row in the payload
QV_HD uint32_t sv_popcount256(const uint8_t *bm) { uint32_t n = 0; for (uint32_t k = 0; k < 8u; k++) n += (uint32_t)__builtin_popcount(qv_le32(bm + 4u * k)); return n; }
QV_HD uint32_t sv_bit(const uint8_t *bm, uint32_t y) { return (bm[y >> 3] >> (y & 7u)) & 1u; }
QV_HD uint32_t sv_row_symbols(const uint32_t *row) { uint32_t n = 0; for (uint32_t y = 0; y < 256u; y++) n += (row[y] & 0xFFFFu) != 0; return n; }
// row (frequency | cumulative << 16) -> its bitmap and frequencies at o; -> the bytes written, 32 + 2 symbols
QV_HD uint32_t sv_put_row(uint8_t *o, const uint32_t *row)
{
    uint8_t *f = o + 32;
    for (uint32_t k = 0; k < 32u; k++) {
        uint32_t bits = 0;
        for (uint32_t j = 0; j < 8u; j++) { const uint32_t v = row[8u * k + j] & 0xFFFFu; if (v) { bits |= 1u << j; *f++ = (uint8_t)v; *f++ = (uint8_t)(v >> 8); } }
        o[k] = (uint8_t)bits;
    }
    return (uint32_t)(f - o);
}
// ... and back: the row at r (the head check has seen that it lies in the payload) -> row[256]
QV_HD int sv_load_row(const uint8_t *r, uint32_t *row)
{
    const uint8_t *f = r + 32;
    uint32_t c = 0;
    for (uint32_t y = 0; y < 256u; y++) {
        uint32_t v = 0;
        if (sv_bit(r, y)) { v = (uint32_t)f[0] | ((uint32_t)f[1] << 8); f += 2; if (v < 1u || v > QV_TOT || c + v > QV_TOT) return SV_E_ROW; }
        row[y] = v | (c << 16); c += v;
    }
    return c == QV_TOT ? SV_OK : SV_E_ROW;
}
QV_HD void sv_clear_row(uint32_t *row) { for (uint32_t y = 0; y < 256u; y++) row[y] = 0; }

// ---------------------------------------------------------------------------------------------------------------- the coder over a strand
// the n bytes at tx, last to first, into [slab_lo, slab_hi) downwards from slab_hi.  order1: tab holds 256 rows and the row is the byte in front, 0 for the
// first.  -> its bytes (they end at slab_hi), 0 without text, QV_SLAB_OVERFLOW when the slab is too small or a byte has no frequency (never)
QV_HD uint32_t sv_strand_encode(const uint8_t *tx, uint32_t n, const uint32_t *tab, int order1, uint8_t *slab_lo, uint8_t *slab_hi)
{
    if (!n) return 0;
    uint32_t x = QV_LOW, y = tx[n - 1u]; uint8_t *p = slab_hi;
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t ctx = i ? tx[i - 1u] : 0u, e = tab[order1 ? (ctx << 8) | y : y];
        if (p - slab_lo < 6 || !(e & 0xFFFFu)) return QV_SLAB_OVERFLOW;
        qv_enc_step(x, e, p);
        y = ctx;
    }
    p -= 4;
    p[0] = (uint8_t)(x >> 24); p[1] = (uint8_t)(x >> 16); p[2] = (uint8_t)(x >> 8); p[3] = (uint8_t)x;
    return (uint32_t)(slab_hi - p);
}
// ... and back: the len bytes at src -> the n bytes at out, no more and no fewer.  *crc: the CRC-32 of what was written (0 without text)
QV_HD int sv_strand_decode(const uint8_t *src, uint32_t len, const uint32_t *tab, int order1, uint8_t *out, uint32_t n, const uint32_t *crctab, uint32_t *crc)
{
    *crc = 0;
    if (!n) return len ? SV_E_SHORT : SV_OK;
    if (len < 4u) return SV_E_SHORT;
    const uint8_t *p = src + 4, *end = src + len;
    uint32_t x = ((uint32_t)src[0] << 24) | ((uint32_t)src[1] << 16) | ((uint32_t)src[2] << 8) | (uint32_t)src[3];
    if (x < QV_LOW) return SV_E_END;
    uint32_t ctx = 0, c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t y;
        const int e = qv_dec_step(x, tab + (order1 ? ctx << 8 : 0u), 256u, p, end, &y);
        if (e) return e;
        out[i] = (uint8_t)y;
        c = crctab[(c ^ y) & 0xFFu] ^ (c >> 8);
        ctx = y;
    }
    *crc = c ^ 0xFFFFFFFFu;
    return x == QV_LOW && p == end ? SV_OK : SV_E_END;
}

// ---------------------------------------------------------------------------------------------------------------- prefix and head
// The prefix of a block, u32 payload_bytes and the mode, block_text_bytes and crc32 that every payload starts with, at q with `left` bytes of the packed form
// from q on (fewer than SV_PREFIX: none of q is read): -> 1 with the size of a payload that holds its head and fits what is left behind the u32, and the text
// bytes when they are `want`, the block's share of the text; or 0
QV_HD int sv_prefix(const uint8_t *q, uint64_t left, uint32_t want, uint64_t *payload_bytes, uint64_t *text_bytes)
{
    if (left < SV_PREFIX) return 0;
    *payload_bytes = qv_le32(q); *text_bytes = qv_le32(q + 5);
    return *payload_bytes >= SV_HEAD0 && *payload_bytes <= left - 4u && *text_bytes == want;
}
// The head of a payload of pbytes bytes for a block of m text bytes, looked at by one lane: -> SV_OK with *mode and *crc, and for the coded modes *hdr, the
// bytes in front of the strands, and rowoff[256]: where in the payload the row of every previous byte starts (mode 1: rowoff[0] alone), 0 for an absent row.
// Every row named there lies in the payload with its bitmap and its frequencies
QV_HD int sv_check_head(const uint8_t *pl, uint32_t pbytes, uint32_t m, uint32_t *mode, uint32_t *crc, uint32_t *hdr, uint32_t *rowoff)
{
    if (pbytes < SV_HEAD0) return SV_E_SIZE;
    *mode = pl[0]; *crc = qv_le32(pl + 5);
    if (pl[0] > 2u) return SV_E_MODE;
    if (qv_le32(pl + 1) != m) return SV_E_SIZE;
    if (pl[0] == 0) return pbytes - SV_HEAD0 == m ? SV_OK : SV_E_SIZE;
    if (pbytes < SV_TAB0) return SV_E_SIZE;
    if (!sv_popcount256(pl + SV_HEAD0)) return SV_E_BITMAP;
    uint32_t at;
    if (pl[0] == 1u) { rowoff[0] = SV_HEAD0; at = SV_TAB0 + 2u * sv_popcount256(pl + SV_HEAD0); }
    else {
        at = SV_TAB0;
        for (uint32_t r = 0; r < 256u; r++) {
            rowoff[r] = 0;
            if (!sv_bit(pl + SV_HEAD0, r)) continue;
            if (pbytes - at < 32u) return SV_E_SIZE;
            const uint32_t A = sv_popcount256(pl + at);
            if (!A) return SV_E_BITMAP;
            if (pbytes - at - 32u < 2u * A) return SV_E_SIZE;
            rowoff[r] = at; at += 32u + 2u * A;
        }
    }
    if (at > pbytes || pbytes - at < SV_LENS) return SV_E_SIZE;
    *hdr = at + SV_LENS;
    return SV_OK;
}
// strand s of a coded payload whose strands start at hdr: its coded bytes as the head announces them
QV_HD int sv_check_strand(const uint8_t *pl, uint32_t hdr, uint32_t m, uint32_t s, uint32_t *slen)
{
    *slen = qv_le32(pl + hdr - SV_LENS + 4u * s);
    return (sv_strand_bytes(m, s) ? *slen < 4u : *slen != 0u) ? SV_E_SHORT : SV_OK;
}
// the CRC-32 of a text from those of its strands: c is the CRC of strand s of a block of m bytes -> its term of the sum (XOR) over the strands
QV_HD uint32_t sv_crc_term(uint32_t c, uint32_t m, uint32_t s) { return dm_gfmul(c, dm_xpow8(m - sv_strand_at(m, s + 1u))); }

// ---------------------------------------------------------------------------------------------------------------- one block on the host, in a row
struct SvWork {
    uint32_t t0[256], t1[65536];
    uint32_t rowoff[256], len1[SV_STRANDS], len2[SV_STRANDS], crctab[256];
};
// bytes a caller must hand to sv_block_encode as `slabs` for a block of m bytes: every strand coded both ways
QV_HD uint64_t sv_block_slabs(uint32_t m) { return 2ull * SV_STRANDS * sv_slab_bytes(m); }

// the m >= 1 bytes at text -> u32 payload_bytes and the payload at out.  -> the bytes of the block (13 + m at most), 0 when cap is smaller (nothing is written
// then) or a slab overflowed (never).  *mode: the mode chosen
QV_HD uint32_t sv_block_encode(const uint8_t *text, uint32_t m, SvWork &W, uint8_t *slabs, uint8_t *out, uint64_t cap, int *mode)
{
    for (uint32_t i = 0; i < 256u; i++) { W.crctab[i] = im_crc_entry(i); W.t0[i] = 0; }
    for (uint32_t i = 0; i < 65536u; i++) W.t1[i] = 0;
    const uint32_t crc = dm_crc_bytes(text, m, W.crctab), slab = sv_slab_bytes(m);
    for (uint32_t s = 0; s < SV_STRANDS; s++) {
        const uint32_t a = sv_strand_at(m, s), n = sv_strand_bytes(m, s);
        uint32_t prev = 0;
        for (uint32_t i = 0; i < n; i++) { const uint32_t v = text[a + i]; W.t0[v]++; W.t1[(prev << 8) | v]++; prev = v; }
    }
    (void)id_norm_counts(W.t0, 256u);
    uint32_t h1 = SV_TAB0 + 2u * sv_row_symbols(W.t0) + SV_LENS, h2 = SV_TAB0 + SV_LENS;
    for (uint32_t r = 0; r < 256u; r++) if (id_norm_counts(W.t1 + 256u * r, 256u)) h2 += 32u + 2u * sv_row_symbols(W.t1 + 256u * r);
    uint64_t total1 = 0, total2 = 0;
    for (uint32_t s = 0; s < SV_STRANDS; s++) {
        const uint32_t a = sv_strand_at(m, s), n = sv_strand_bytes(m, s);
        uint8_t *lo1 = slabs + (uint64_t)s * slab, *lo2 = slabs + (uint64_t)(SV_STRANDS + s) * slab;
        W.len1[s] = sv_strand_encode(text + a, n, W.t0, 0, lo1, lo1 + slab);
        W.len2[s] = sv_strand_encode(text + a, n, W.t1, 1, lo2, lo2 + slab);
        if (W.len1[s] == QV_SLAB_OVERFLOW || W.len2[s] == QV_SLAB_OVERFLOW) return 0;
        total1 += W.len1[s]; total2 += W.len2[s];
    }
    const uint32_t md = sv_choose(m, h1 + total1, h2 + total2);
    if (mode) *mode = (int)md;
    const uint32_t payload = md == 0 ? SV_HEAD0 + m : md == 1u ? h1 + (uint32_t)total1 : h2 + (uint32_t)total2;
    if (cap < 4ull + payload) return 0;
    qv_put32(out, payload);
    uint8_t *o = out + 4;
    o[0] = (uint8_t)md; qv_put32(o + 1, m); qv_put32(o + 5, crc);
    o += SV_HEAD0;
    if (md == 0) { for (uint32_t i = 0; i < m; i++) o[i] = text[i]; return 4u + payload; }
    if (md == 1u) o += sv_put_row(o, W.t0);
    else {
        uint8_t *rows = o + 32;
        for (uint32_t k = 0; k < 32u; k++) o[k] = 0;
        for (uint32_t r = 0; r < 256u; r++) if (sv_row_symbols(W.t1 + 256u * r)) { o[r >> 3] |= (uint8_t)(1u << (r & 7u)); rows += sv_put_row(rows, W.t1 + 256u * r); }
        o = rows;
    }
    const uint32_t *len = md == 1u ? W.len1 : W.len2;
    for (uint32_t s = 0; s < SV_STRANDS; s++) { qv_put32(o, len[s]); o += 4; }
    for (uint32_t s = 0; s < SV_STRANDS; s++) {
        const uint8_t *src = slabs + (uint64_t)((md == 1u ? 0u : SV_STRANDS) + s + 1u) * slab - len[s];
        for (uint32_t i = 0; i < len[s]; i++) *o++ = src[i];
    }
    return 4u + payload;
}

// the payload of a block of m text bytes (pbytes bytes, behind its u32) -> its text at text.  Reads only the payload, writes only the m bytes.  Of everything
// that is wrong in the rows and the strand sizes, and then in the strands, the smallest code is the answer: the lanes of a workgroup agree on it in any order
QV_HD int sv_block_decode(const uint8_t *pl, uint32_t pbytes, uint32_t m, SvWork &W, uint8_t *text)
{
    uint32_t mode = 0, crc = 0, hdr = 0;
    const int e = sv_check_head(pl, pbytes, m, &mode, &crc, &hdr, W.rowoff);
    if (e) return e;
    for (uint32_t i = 0; i < 256u; i++) W.crctab[i] = im_crc_entry(i);
    if (mode == 0) {
        for (uint32_t i = 0; i < m; i++) text[i] = pl[SV_HEAD0 + i];
        return dm_crc_bytes(text, m, W.crctab) == crc ? SV_OK : SV_E_CRC;
    }
    uint32_t bad = SV_E_NONE;
    if (mode == 1u) bad = id_min(bad, sv_code(sv_load_row(pl + W.rowoff[0], W.t0)));
    else for (uint32_t r = 0; r < 256u; r++) { if (W.rowoff[r]) bad = id_min(bad, sv_code(sv_load_row(pl + W.rowoff[r], W.t1 + 256u * r))); else sv_clear_row(W.t1 + 256u * r); }
    uint64_t lsum = 0;
    for (uint32_t s = 0; s < SV_STRANDS; s++) { bad = id_min(bad, sv_code(sv_check_strand(pl, hdr, m, s, &W.len1[s]))); lsum += W.len1[s]; }
    if (lsum != pbytes - hdr) bad = id_min(bad, SV_E_LENGTHS);
    if (bad != SV_E_NONE) return (int)bad;
    const uint8_t *src = pl + hdr;
    for (uint32_t s = 0; s < SV_STRANDS; s++) {
        uint32_t c;
        bad = id_min(bad, sv_code(sv_strand_decode(src, W.len1[s], mode == 1u ? W.t0 : W.t1, mode == 2u, text + sv_strand_at(m, s), sv_strand_bytes(m, s), W.crctab, &c)));
        src += W.len1[s];
    }
    if (bad != SV_E_NONE) return (int)bad;
    return dm_crc_bytes(text, m, W.crctab) == crc ? SV_OK : SV_E_CRC;
}
