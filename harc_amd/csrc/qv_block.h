// qv_block.h -- one block of the packed quality file X.quality.hq (README: "The packed quality file"): m lines of L quality values -> u32 payload_bytes and the
// payload, stored (mode 0) or coded (mode 1) with order-1 static rANS in 256 strands.  Every function that decides a byte of a block lives here once: qpack.hip
// runs them on the device (a workgroup per block, a lane per strand), harc_amd_qpack_host / harc_amd_qunpack_host run them in a row on the host, and
// tests/test_qpack_host.py builds this file with g++ and sanitizers as a stand-alone program.  No local arrays: on the device they would live in private memory.
//
// The table.  Symbols are the distinct bytes of the block in ascending order, 0 .. A-1; the context of a symbol is the symbol in front of it in its line, row A
// is the context of a line's first column.  One u32 per (context, symbol) at fc[context * A + symbol]: first the count, then the frequency (qv_norm_row), then
// frequency | cumulative << 16 (qv_cum_row).  The file stores the frequencies as u16.
//
// Normalising a row of counts c[0 .. A) with T = sum c to 4096 -- the encoder's one rule, host and device:
//     f[y] = max(1, floor(c[y] * 4096 / T)) for c[y] > 0, 0 otherwise;   then f[b] += 4096 - sum f, b = the largest count, the lowest symbol on ties.
// f[b] stays >= 1: let k entries be lifted to 1 (their c * 4096 / T < 1, together < k).  The other A - k entries share more than 4096 - k, so the largest
// count has c[b] * 4096 / T > (4096 - k) / (A - k) and f[b] > (4096 - k) / (A - k) - 1 before the correction.  sum of the floors <= 4096, so the correction
// takes at most k away: f[b] > (4096 - k) / (A - k) - 1 - k, which over 0 <= k < A <= 94 is smallest near k = 32, A = 94 (65.5 - 33 = 32.5).  A positive
// correction only adds.
//
// The coder: 32-bit rANS, 12 probability bits, bytes, lower bound 2^23.  The encoder starts a strand at 2^23 and walks its symbols last to first, writing the
// bytes it shifts out DOWNWARDS; the four bytes of the final state go in front, most significant first.  A step adds at most 12 + log2(1 + 2^-11) bits, so a
// strand of s symbols is at most 1.5 s + s / 2048 + 4 bytes (qv_slab_bytes leaves more; the encoder still checks before it writes).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QV_HD __host__ __device__ __forceinline__
#else
#define QV_HD static inline
#endif

enum {
    QV_OK = 0,
    QV_E_MODE = 1,         // the mode byte is neither 0 nor 1
    QV_E_SIZE = 2,         // a stored payload that is not 1 + m * L bytes; a coded one shorter than its header and table
    QV_E_ALPHABET = 3,     // A outside 1..94, or not the number of bits set in the bitmap
    QV_E_ROW = 4,          // a row of frequencies that sums to neither 0 nor 4096
    QV_E_LENGTHS = 5,      // the strand lengths do not sum to the rest of the payload
    QV_E_SHORT = 6,        // a strand with lines shorter than 4 bytes, or a strand without lines that is not empty
    QV_E_TRUNC = 7,        // the decoder needs a byte behind the strand's end
    QV_E_CONTEXT = 8,      // a slot that belongs to no symbol of the row: a context whose row is all zero
    QV_E_END = 9,          // the state is not 2^23 or the strand has bytes left after its last symbol (or its first state is below 2^23)
};

#define QV_TOT 4096u
#define QV_LOW (1u << 23)
#define QV_STRANDS 256u
#define QV_MAXA 94u
#define QV_FIRST 33u                                   // byte value of bit 0 of the bitmap
#define QV_TABLE ((QV_MAXA + 1u) * QV_MAXA)
#define QV_FILE_HEADER 32u
#define QV_MAX_BLOCK_SYMBOLS (1u << 30)                // reads per block x read length: the payload size is a u32
#define QV_SLAB_OVERFLOW 0xFFFFFFFFu
#define QV_E_NONE 0xFFFFFFFFu                          // qv_code(QV_OK): what a minimum over codes starts from

QV_HD uint32_t qv_default_rb(uint32_t L) { const uint32_t r = (1u << 22) / L; return r < 256u ? 256u : r; }
QV_HD uint64_t qv_blocks(uint64_t n, uint32_t rb) { return rb ? (n + rb - 1) / rb : 0; }
QV_HD uint64_t qv_bound(uint64_t n, uint32_t L, uint32_t rb) { return QV_FILE_HEADER + qv_blocks(n, rb) * 5u + n * L; }
QV_HD uint32_t qv_hdr1(uint32_t A) { return 14u + 2u * (A + 1u) * A + 4u * QV_STRANDS; }        // mode, A, bitmap, table, strand lengths
QV_HD uint32_t qv_strand_lines(uint32_t m, uint32_t s) { return s < m ? (m - s + QV_STRANDS - 1u) / QV_STRANDS : 0u; }
// scratch for one strand of nsym symbols, a multiple of 16
QV_HD uint32_t qv_slab_bytes(uint32_t nsym) { return ((3u * (nsym >> 1)) + (nsym >> 10) + 2u + 16u + 15u) & ~15u; }
QV_HD uint32_t qv_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
QV_HD uint32_t qv_code(int e) { return e ? (uint32_t)e : QV_E_NONE; }
QV_HD uint32_t qv_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
QV_HD void qv_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
QV_HD void qv_put64(uint8_t *p, uint64_t v) { qv_put32(p, (uint32_t)v); qv_put32(p + 4, (uint32_t)(v >> 32)); }
QV_HD uint64_t qv_le64(const uint8_t *p) { return (uint64_t)qv_le32(p) | ((uint64_t)qv_le32(p + 4) << 32); }
QV_HD void qv_file_header(uint8_t *h, uint32_t L, uint32_t rb, uint64_t n)
{
    h[0] = 'H'; h[1] = 'A'; h[2] = 'R'; h[3] = 'C'; h[4] = 'Q'; h[5] = '1'; h[6] = 0; h[7] = 0;
    qv_put32(h + 8, L); qv_put32(h + 12, rb); qv_put64(h + 16, n); qv_put64(h + 24, 0);
}
QV_HD int qv_magic_ok(const uint8_t *h) { return h[0] == 'H' && h[1] == 'A' && h[2] == 'R' && h[3] == 'C' && h[4] == 'Q' && h[5] == '1' && h[6] == 0 && h[7] == 0; }

// ---------------------------------------------------------------------------------------------------------------- the symbol map
// bm[3]: bit k set when byte 33 + k occurs.  The symbol of byte 33 + k is the number of set bits below bit k
QV_HD uint32_t qv_bit(const uint32_t *bm, uint32_t k) { return (bm[k >> 5] >> (k & 31u)) & 1u; }
QV_HD uint32_t qv_rank(const uint32_t *bm, uint32_t k)              // k <= 96
{
    uint32_t r = 0;
    for (uint32_t w = 0; w < (k >> 5); w++) r += (uint32_t)__builtin_popcount(bm[w]);
    if (k & 31u) r += (uint32_t)__builtin_popcount(bm[k >> 5] & ((1u << (k & 31u)) - 1u));
    return r;
}
// sym_of[k] for k < 94 (any value where the bit is clear), byte_of[symbol]
QV_HD void qv_map_entry(const uint32_t *bm, uint32_t k, uint8_t *sym_of, uint8_t *byte_of)
{
    const uint32_t r = qv_rank(bm, k);
    sym_of[k] = (uint8_t)r;
    if (qv_bit(bm, k)) byte_of[r] = (uint8_t)(QV_FIRST + k);
}

// ---------------------------------------------------------------------------------------------------------------- the table
QV_HD void qv_norm_row(uint32_t *row, uint32_t A)
{
    uint64_t T = 0; uint32_t best = 0, bi = 0;
    for (uint32_t y = 0; y < A; y++) { const uint32_t c = row[y]; T += c; if (c > best) { best = c; bi = y; } }
    if (!T) return;
    uint32_t sum = 0;
    for (uint32_t y = 0; y < A; y++) {
        const uint32_t c = row[y];
        if (!c) continue;
        uint32_t f = (uint32_t)(((uint64_t)c << 12) / T);
        if (!f) f = 1;
        row[y] = f; sum += f;
    }
    row[bi] = row[bi] + QV_TOT - sum;
}
QV_HD void qv_cum_row(uint32_t *row, uint32_t A)
{
    uint32_t c = 0;
    for (uint32_t y = 0; y < A; y++) { const uint32_t f = row[y]; row[y] = f | (c << 16); c += f; }
}
// row r of the stored table (u16 frequencies at tab) -> row[] as frequency | cumulative << 16; the sum must be 0 or 4096
QV_HD int qv_load_row(const uint8_t *tab, uint32_t r, uint32_t A, uint32_t *row)
{
    const uint8_t *p = tab + 2u * r * A;
    uint32_t c = 0;
    for (uint32_t y = 0; y < A; y++) {
        const uint32_t f = (uint32_t)p[2 * y] | ((uint32_t)p[2 * y + 1] << 8);
        if (f > QV_TOT || c + f > QV_TOT) return QV_E_ROW;
        row[y] = f | (c << 16); c += f;
    }
    return c == 0 || c == QV_TOT ? QV_OK : QV_E_ROW;
}

// ---------------------------------------------------------------------------------------------------------------- the coder
// e = frequency | cumulative << 16 of the symbol in its context; at most two bytes leave, at p - 1 and p - 2
QV_HD void qv_enc_step(uint32_t &x, uint32_t e, uint8_t *&p)
{
    const uint32_t f = e & 0xFFFFu, c = e >> 16, xmax = f << 19;     // ((2^23 >> 12) << 8) * f; 2^31 for f = 4096
    while (x >= xmax) { *--p = (uint8_t)x; x >>= 8; }
    x = ((x / f) << 12) + (x % f) + c;
}
QV_HD int qv_dec_step(uint32_t &x, const uint32_t *row, uint32_t A, const uint8_t *&p, const uint8_t *end, uint32_t *y_out)
{
    const uint32_t slot = x & (QV_TOT - 1u);
    uint32_t lo = 0, hi = A - 1u;                                   // the last symbol whose cumulative is <= slot: symbols without frequency share theirs with the next one
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if ((row[mid] >> 16) <= slot) lo = mid; else hi = mid - 1u; }
    const uint32_t e = row[lo], f = e & 0xFFFFu, c = e >> 16;
    if (slot - c >= f) return QV_E_CONTEXT;
    x = f * (x >> 12) + slot - c;                                   // < 2^32: f <= 4096, x >> 12 < 2^20, slot - c < f
    while (x < QV_LOW) { if (p == end) return QV_E_TRUNC; x = (x << 8) | *p++; }
    *y_out = lo;
    return QV_OK;
}

// Strand s of a block: lines s, s + 256, ... of the m lines at text (stride L + 1), coded from the last symbol of the last line to the first of the first into
// [slab_lo, slab_hi), downwards from slab_hi.  -> its bytes (they end at slab_hi), 0 for a strand without lines, QV_SLAB_OVERFLOW when the slab is too small (never)
QV_HD uint32_t qv_strand_encode(const uint8_t *text, uint32_t L, uint32_t m, uint32_t s, const uint32_t *fc, uint32_t A, const uint8_t *sym_of, uint8_t *slab_lo,
                                uint8_t *slab_hi)
{
    const uint32_t nl = qv_strand_lines(m, s);
    if (!nl) return 0;
    uint32_t x = QV_LOW; uint8_t *p = slab_hi;
    for (uint32_t k = nl; k-- > 0;) {
        const uint8_t *ln = text + (uint64_t)(s + k * QV_STRANDS) * (L + 1u);
        uint32_t y = sym_of[ln[L - 1u] - QV_FIRST];
        for (uint32_t j = L; j-- > 0;) {
            const uint32_t ctx = j ? sym_of[ln[j - 1u] - QV_FIRST] : A;
            const uint32_t e = fc[ctx * A + y];
            if (p - slab_lo < 6 || !(e & 0xFFFFu)) return QV_SLAB_OVERFLOW;      // (a pair without a frequency: the table is not this text's)
            qv_enc_step(x, e, p);
            y = ctx;
        }
    }
    p -= 4;
    p[0] = (uint8_t)(x >> 24); p[1] = (uint8_t)(x >> 16); p[2] = (uint8_t)(x >> 8); p[3] = (uint8_t)x;
    return (uint32_t)(slab_hi - p);
}
// ... and back: the len bytes at src -> lines s, s + 256, ... of out (stride L + 1), a newline behind each
QV_HD int qv_strand_decode(const uint8_t *src, uint32_t len, const uint32_t *fc, uint32_t A, const uint8_t *byte_of, uint8_t *out, uint32_t L, uint32_t m, uint32_t s)
{
    const uint32_t nl = qv_strand_lines(m, s);
    if (!nl) return len ? QV_E_SHORT : QV_OK;
    if (len < 4) return QV_E_SHORT;
    const uint8_t *p = src + 4, *end = src + len;
    uint32_t x = ((uint32_t)src[0] << 24) | ((uint32_t)src[1] << 16) | ((uint32_t)src[2] << 8) | (uint32_t)src[3];
    if (x < QV_LOW) return QV_E_END;
    for (uint32_t k = 0; k < nl; k++) {
        uint8_t *ln = out + (uint64_t)(s + k * QV_STRANDS) * (L + 1u);
        uint32_t ctx = A;
        for (uint32_t j = 0; j < L; j++) {
            uint32_t y;
            const int e = qv_dec_step(x, fc + ctx * A, A, p, end, &y);
            if (e) return e;
            ln[j] = byte_of[y];
            ctx = y;
        }
        ln[L] = '\n';
    }
    return x == QV_LOW && p == end ? QV_OK : QV_E_END;
}

// ---------------------------------------------------------------------------------------------------------------- stored or coded
QV_HD int qv_in_alphabet(uint32_t v) { return v - QV_FIRST < QV_MAXA; }
// a block whose bytes all lie in 33..126 is coded when that is smaller
QV_HD int qv_use_coded(uint32_t A, uint32_t strand_bytes, uint32_t m, uint32_t L) { return qv_hdr1(A) + strand_bytes < 1u + m * L; }

// The prefix of a block, u32 payload_bytes, at q with `left` bytes of the packed form from q on (fewer than QV_PREFIX: none of q is read): -> 1 with the size of a
// payload that is not empty and fits what is left behind the prefix, or 0
#define QV_PREFIX 4u
QV_HD int qv_prefix(const uint8_t *q, uint64_t left, uint64_t *payload_bytes)
{
    if (left < QV_PREFIX) return 0;
    *payload_bytes = qv_le32(q);
    return *payload_bytes >= 1 && *payload_bytes <= left - QV_PREFIX;
}
// the head of a payload of pbytes bytes for m lines of L: -> QV_OK with *mode, and for mode 1 *A and bm[3]
QV_HD int qv_check_head(const uint8_t *pl, uint32_t pbytes, uint32_t m, uint32_t L, uint32_t *mode, uint32_t *A, uint32_t *bm)
{
    if (pbytes < 1) return QV_E_SIZE;
    *mode = pl[0];
    if (pl[0] == 0) return (uint64_t)pbytes == 1ull + (uint64_t)m * L ? QV_OK : QV_E_SIZE;
    if (pl[0] != 1) return QV_E_MODE;
    if (pbytes < 14) return QV_E_SIZE;
    const uint32_t a = pl[1];
    bm[0] = qv_le32(pl + 2); bm[1] = qv_le32(pl + 6); bm[2] = qv_le32(pl + 10);
    if (a < 1 || a > QV_MAXA || (bm[2] >> 30) || qv_rank(bm, 96) != a) return QV_E_ALPHABET;
    if (pbytes < qv_hdr1(a)) return QV_E_SIZE;
    *A = a;
    return QV_OK;
}

// ---------------------------------------------------------------------------------------------------------------- one block on the host, in a row
struct QvWork {
    uint32_t fc[QV_TABLE];
    uint32_t bm[3];
    uint32_t len[QV_STRANDS];
    uint8_t sym_of[96], byte_of[96];
};
// bytes a caller must hand to qv_block_encode as `slabs` for a block of m lines of L
QV_HD uint64_t qv_block_slabs(uint32_t m, uint32_t L) { return (uint64_t)QV_STRANDS * qv_slab_bytes(qv_strand_lines(m, 0) * L); }

// m lines of L (stride L + 1; only the m * (L + 1) bytes at text are read, the newlines not looked at) -> u32 payload_bytes and the payload at out.
// -> the bytes of the block (5 + m * L at most), 0 when cap is smaller (nothing is written then) or a slab overflowed (never).  *stored: the mode was 0
QV_HD uint32_t qv_block_encode(const uint8_t *text, uint32_t m, uint32_t L, QvWork &W, uint8_t *slabs, uint8_t *out, uint64_t cap, int *stored)
{
    const uint32_t stored_bytes = 4u + 1u + m * L;
    int coded = 1; uint32_t A = 0, total = 0;
    W.bm[0] = W.bm[1] = W.bm[2] = 0;
    for (uint32_t i = 0; i < m && coded; i++) {
        const uint8_t *ln = text + (uint64_t)i * (L + 1u);
        for (uint32_t j = 0; j < L; j++) { const uint32_t k = ln[j] - QV_FIRST; if (k >= QV_MAXA) { coded = 0; break; } W.bm[k >> 5] |= 1u << (k & 31u); }
    }
    const uint32_t slab = qv_slab_bytes(qv_strand_lines(m, 0) * L);
    if (coded) {
        A = qv_rank(W.bm, 96);
        for (uint32_t k = 0; k < QV_MAXA; k++) qv_map_entry(W.bm, k, W.sym_of, W.byte_of);
        for (uint32_t i = 0; i < (A + 1u) * A; i++) W.fc[i] = 0;
        for (uint32_t i = 0; i < m; i++) {
            const uint8_t *ln = text + (uint64_t)i * (L + 1u);
            uint32_t ctx = A;
            for (uint32_t j = 0; j < L; j++) { const uint32_t y = W.sym_of[ln[j] - QV_FIRST]; W.fc[ctx * A + y]++; ctx = y; }
        }
        for (uint32_t r = 0; r <= A; r++) { qv_norm_row(W.fc + r * A, A); qv_cum_row(W.fc + r * A, A); }
        for (uint32_t s = 0; s < QV_STRANDS; s++) {
            uint8_t *lo = slabs + (uint64_t)s * slab;
            const uint32_t n = qv_strand_encode(text, L, m, s, W.fc, A, W.sym_of, lo, lo + slab);
            if (n == QV_SLAB_OVERFLOW) return 0;
            W.len[s] = n; total += n;
        }
        coded = qv_use_coded(A, total, m, L);
    }
    if (stored) *stored = !coded;
    if (!coded) {
        if (cap < stored_bytes) return 0;
        qv_put32(out, stored_bytes - 4u);
        out[4] = 0;
        uint8_t *o = out + 5;
        for (uint32_t i = 0; i < m; i++) { const uint8_t *ln = text + (uint64_t)i * (L + 1u); for (uint32_t j = 0; j < L; j++) *o++ = ln[j]; }
        return stored_bytes;
    }
    const uint32_t size = 4u + qv_hdr1(A) + total;
    if (cap < size) return 0;
    qv_put32(out, size - 4u);
    uint8_t *o = out + 4;
    o[0] = 1; o[1] = (uint8_t)A;
    qv_put32(o + 2, W.bm[0]); qv_put32(o + 6, W.bm[1]); qv_put32(o + 10, W.bm[2]);
    o += 14;
    for (uint32_t i = 0; i < (A + 1u) * A; i++) { const uint32_t f = W.fc[i] & 0xFFFFu; *o++ = (uint8_t)f; *o++ = (uint8_t)(f >> 8); }
    for (uint32_t s = 0; s < QV_STRANDS; s++) { qv_put32(o, W.len[s]); o += 4; }
    for (uint32_t s = 0; s < QV_STRANDS; s++) {
        const uint8_t *src = slabs + (uint64_t)(s + 1u) * slab - W.len[s];
        for (uint32_t i = 0; i < W.len[s]; i++) *o++ = src[i];
    }
    return size;
}

// the payload of a block (pbytes bytes, behind its u32) -> the m * (L + 1) bytes of its lines at text.  Reads only the payload, writes only the lines.  Of
// everything that is wrong in the rows and the strand lengths, and then in the strands, the smallest code is the answer: the lanes of a workgroup agree on it
// in any order
QV_HD int qv_block_decode(const uint8_t *pl, uint32_t pbytes, uint32_t m, uint32_t L, QvWork &W, uint8_t *text)
{
    uint32_t mode = 0, A = 0;
    const int e = qv_check_head(pl, pbytes, m, L, &mode, &A, W.bm);
    if (e) return e;
    if (mode == 0) {
        const uint8_t *p = pl + 1;
        for (uint32_t i = 0; i < m; i++) { uint8_t *ln = text + (uint64_t)i * (L + 1u); for (uint32_t j = 0; j < L; j++) ln[j] = *p++; ln[L] = '\n'; }
        return QV_OK;
    }
    for (uint32_t k = 0; k < QV_MAXA; k++) qv_map_entry(W.bm, k, W.sym_of, W.byte_of);
    uint32_t bad = QV_E_NONE;
    for (uint32_t r = 0; r <= A; r++) bad = qv_min(bad, qv_code(qv_load_row(pl + 14, r, A, W.fc + r * A)));
    const uint32_t h = qv_hdr1(A), rest = pbytes - h;
    const uint8_t *lens = pl + h - 4u * QV_STRANDS;
    uint64_t sum = 0;
    for (uint32_t s = 0; s < QV_STRANDS; s++) {
        const uint32_t n = qv_le32(lens + 4u * s);
        if (qv_strand_lines(m, s) ? n < 4 : n != 0) bad = qv_min(bad, QV_E_SHORT);
        W.len[s] = n; sum += n;
    }
    if (sum != rest) bad = qv_min(bad, QV_E_LENGTHS);
    if (bad != QV_E_NONE) return (int)bad;
    const uint8_t *src = pl + h;
    for (uint32_t s = 0; s < QV_STRANDS; s++) {
        bad = qv_min(bad, qv_code(qv_strand_decode(src, W.len[s], W.fc, A, W.byte_of, text, L, m, s)));
        src += W.len[s];
    }
    return bad == QV_E_NONE ? QV_OK : (int)bad;
}
