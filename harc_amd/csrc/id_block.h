// id_block.h -- one block of the packed id file X.id.hi (README: "The packed id file"): m lines of an id text -> u32 payload_bytes and the payload, stored
// (mode 0) or coded (mode 1): every line against the line in front of it in its strand, token by token, as events of a static rANS stream per strand.  Every
// function that decides a byte of a block lives here once: idpack.hip runs them on the device (a workgroup per block, a lane per strand),
// harc_amd_idpack_host / harc_amd_idunpack_host run them in a row on the host, and tests/test_idpack_host.py builds this file with g++ and sanitizers as a
// stand-alone program.  No local arrays: on the device they would live in private memory.  The coder, the row normaliser and the little-endian helpers are
// qv_block.h's.
//
// Strands.  q = ceil(m / 256); strand s holds the consecutive lines [s q, min(m, (s + 1) q)) and is coded against itself only: its first line against an
// empty line.  A strand is therefore one piece of the text, and a lane finds its lines by looking for newlines.
//
// Tokens.  A line is cut into maximal runs of ASCII digits and maximal runs of other bytes.  A digit run of at most 9 digits without a leading zero (or a single
// 0) is numeric; everything else is a string.  Token t is coded against token t of the previous line.
//
// Events, each a symbol in a row of the table (frequency | cumulative << 16 once normalised; 124 rows, 12 368 entries):
//     rows   0 ..  15   op[min(t, 15)]      5 symbols: 0 MATCH, 1 DELTA, 2 NUM, 3 STR, 4 END
//     rows  16 ..  23   delta[min(t, 7)]    256 symbols: cur - prev, 1 .. 255
//     rows  24 ..  27   num[k]              256 symbols: byte k of the value, low byte first
//     rows  28 .. 123   str[previous symbol of the literal, 0 at its start]   96 symbols: byte - 31 (1 .. 95), 0 ends the literal
// The encoder takes the first op that applies in that order and ends a line with END in row op[min(T, 15)], T its tokens.
//
// The event bound.  A strand whose events number more than its text bytes plus twice its lines is abandoned and its block stored: this bounds the scratch
// (u16 per event, and two bytes of slab per event: a step of the coder adds at most 12 + log2(1 + 2^-11) bits).
#pragma once
#include <stdint.h>
#include "qv_block.h"

enum {
    ID_OK = 0,
    ID_E_MODE = 1,         // the mode byte is neither 0 nor 1
    ID_E_SIZE = 2,         // a payload shorter than its head, a stored one that is not 5 + block_text_bytes, strand text bytes that do not sum to block_text_bytes
    ID_E_BITMAP = 3,       // a bit past the last row is set
    ID_E_ROW = 4,          // a present row that does not sum to 4096
    ID_E_LENGTHS = 5,      // the strand coded bytes do not sum to the rest of the payload
    ID_E_SHORT = 6,        // a strand with lines of fewer than 4 coded bytes or fewer text bytes than lines; a strand without lines that is not empty
    ID_E_TRUNC = 7,        // the decoder needs a byte behind the strand's end                                  (= QV_E_TRUNC)
    ID_E_CONTEXT = 8,      // a slot that belongs to no symbol of the row, or a row that is absent              (= QV_E_CONTEXT)
    ID_E_END = 9,          // the state is not 2^23 or the strand has bytes left after its last line (or its first state is below 2^23)
    ID_E_PREV = 10,        // MATCH without a previous token t, DELTA without a numeric one
    ID_E_VALUE = 11,       // a DELTA of 0, or a DELTA or NUM value above 999 999 999
    ID_E_TEXT = 12,        // a byte or a line that would pass the strand's text bytes, or text bytes or lines that are not met exactly
    ID_E_EMPTY = 13,       // a literal without a byte
};

#define ID_STRANDS 256u
#define ID_ROWS 124u
#define ID_TABLE 12368u
#define ID_ROW_DELTA 16u
#define ID_ROW_NUM 24u
#define ID_ROW_STR 28u
#define ID_OP_MATCH 0u
#define ID_OP_DELTA 1u
#define ID_OP_NUM 2u
#define ID_OP_STR 3u
#define ID_OP_END 4u
#define ID_FILE_HEADER 32u
#define ID_DEFAULT_RB (1u << 18)
#define ID_MAX_BLOCK_TEXT (1u << 30)
#define ID_MAX_VALUE 999999999u
#define ID_NOT_NUMERIC 0xFFFFFFFFu
#define ID_HEAD0 5u                                    // mode, block_text_bytes
#define ID_HEAD1 (ID_HEAD0 + 8u * ID_STRANDS + 16u)    // ... strand text bytes, strand coded bytes, bitmap: the table follows
#define ID_E_NONE 0xFFFFFFFFu                          // id_code(ID_OK): what a minimum over codes starts from
#define ID_EV_OVERFLOW 0xFFFFFFFFu                     // id_strand_events: the event bound was passed
#define ID_EV_BADBYTE 0xFFFFFFFEu                      // ... a byte outside 32..126

QV_HD uint32_t id_row_width(uint32_t r) { return r < ID_ROW_DELTA ? 5u : r < ID_ROW_STR ? 256u : 96u; }
QV_HD uint32_t id_row_off(uint32_t r) { return r < ID_ROW_DELTA ? 5u * r : r < ID_ROW_STR ? 80u + 256u * (r - ID_ROW_DELTA) : 3152u + 96u * (r - ID_ROW_STR); }
QV_HD uint64_t id_blocks(uint64_t n, uint32_t rb) { return rb ? (n + rb - 1) / rb : 0; }
QV_HD uint64_t id_bound(uint64_t text_bytes, uint64_t n, uint32_t rb) { return ID_FILE_HEADER + id_blocks(n, rb) * (4u + ID_HEAD0) + text_bytes; }
QV_HD uint32_t id_strand_q(uint32_t m) { return (m + ID_STRANDS - 1u) / ID_STRANDS; }
// first line of strand s, clamped to m: strands behind the last line hold none
QV_HD uint32_t id_strand_line0(uint32_t m, uint32_t s) { const uint64_t a = (uint64_t)s * id_strand_q(m); return a < m ? (uint32_t)a : m; }
QV_HD uint32_t id_strand_lines(uint32_t m, uint32_t s) { return (s + 1u < ID_STRANDS ? id_strand_line0(m, s + 1u) : m) - id_strand_line0(m, s); }
QV_HD uint32_t id_event_cap(uint32_t text_bytes, uint32_t lines) { return text_bytes + 2u * lines; }
QV_HD uint32_t id_slab_bytes(uint32_t event_cap) { return 2u * event_cap + 32u; }
QV_HD void id_file_header(uint8_t *h, uint32_t rb, uint64_t n, uint64_t text_bytes)
{
    h[0] = 'H'; h[1] = 'A'; h[2] = 'R'; h[3] = 'C'; h[4] = 'I'; h[5] = '1'; h[6] = 0; h[7] = 0;
    qv_put32(h + 8, n ? rb : 0u); qv_put32(h + 12, 0); qv_put64(h + 16, n); qv_put64(h + 24, text_bytes);
}
QV_HD int id_magic_ok(const uint8_t *h) { return h[0] == 'H' && h[1] == 'A' && h[2] == 'R' && h[3] == 'C' && h[4] == 'I' && h[5] == '1' && h[6] == 0 && h[7] == 0; }

// ---------------------------------------------------------------------------------------------------------------- tokens
QV_HD int id_digit(uint32_t b) { return b - 48u < 10u; }
// the token at p, n > 0 bytes before the line's end
QV_HD uint32_t id_tok_len(const uint8_t *p, uint32_t n)
{
    const int d = id_digit(p[0]);
    uint32_t k = 1;
    while (k < n && id_digit(p[k]) == d) k++;
    return k;
}
QV_HD uint32_t id_tok_value(const uint8_t *p, uint32_t len)
{
    if (!id_digit(p[0]) || len > 9u || (p[0] == '0' && len > 1u)) return ID_NOT_NUMERIC;
    uint32_t v = 0;
    for (uint32_t k = 0; k < len; k++) v = v * 10u + (p[k] - 48u);
    return v;
}
// bytes in front of the next newline; n when there is none
QV_HD uint32_t id_line_len(const uint8_t *p, uint32_t n) { uint32_t k = 0; while (k < n && p[k] != '\n') k++; return k; }
QV_HD uint32_t id_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
QV_HD uint32_t id_code(int e) { return e ? (uint32_t)e : 0xFFFFFFFFu; }

// ---------------------------------------------------------------------------------------------------------------- the events of a strand
// counts go into hist (the table before it is normalised): with atomics on the device, where the strands of a block share it
struct IdSink { uint16_t *ev; uint32_t n, cap; uint32_t *hist; };
QV_HD int id_put(IdSink &s, uint32_t row, uint32_t sym)
{
    if (s.n >= s.cap) return 0;
    s.ev[s.n++] = (uint16_t)((row << 8) | sym);
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&s.hist[id_row_off(row) + sym], 1u);
#else
    s.hist[id_row_off(row) + sym]++;
#endif
    return 1;
}
// the nl lines in the tbytes bytes at tx (the last byte is the last line's newline) -> their events at ev (room for cap), counted into hist.
// -> the number of events, ID_EV_OVERFLOW or ID_EV_BADBYTE
QV_HD uint32_t id_strand_events(const uint8_t *tx, uint32_t tbytes, uint32_t nl, uint16_t *ev, uint32_t cap, uint32_t *hist)
{
    IdSink S = { ev, 0u, cap, hist };
    const uint8_t *prev = tx; uint32_t plen = 0, at = 0;
    for (uint32_t i = 0; i < nl; i++) {
        const uint8_t *cur = tx + at;
        const uint32_t clen = id_line_len(cur, tbytes - at);
        uint32_t ci = 0, pi = 0, t = 0;
        while (ci < clen) {
            const uint32_t ct = id_tok_len(cur + ci, clen - ci), hp = pi < plen, pt = hp ? id_tok_len(prev + pi, plen - pi) : 0u, opr = id_min(t, 15u);
            uint32_t same = hp && ct == pt;
            for (uint32_t k = 0; same && k < ct; k++) same = cur[ci + k] == prev[pi + k];
            if (same) { if (!id_put(S, opr, ID_OP_MATCH)) return ID_EV_OVERFLOW; }
            else {
                const uint32_t cv = id_tok_value(cur + ci, ct), pv = hp ? id_tok_value(prev + pi, pt) : ID_NOT_NUMERIC;
                if (cv != ID_NOT_NUMERIC && pv != ID_NOT_NUMERIC && cv > pv && cv - pv <= 255u) {
                    if (!id_put(S, opr, ID_OP_DELTA) || !id_put(S, ID_ROW_DELTA + id_min(t, 7u), cv - pv)) return ID_EV_OVERFLOW;
                } else if (cv != ID_NOT_NUMERIC) {
                    if (!id_put(S, opr, ID_OP_NUM)) return ID_EV_OVERFLOW;
                    for (uint32_t k = 0; k < 4u; k++) if (!id_put(S, ID_ROW_NUM + k, (cv >> (8u * k)) & 255u)) return ID_EV_OVERFLOW;
                } else {
                    if (!id_put(S, opr, ID_OP_STR)) return ID_EV_OVERFLOW;
                    uint32_t ctx = 0;
                    for (uint32_t k = 0; k < ct; k++) {
                        const uint32_t b = cur[ci + k];
                        if (b - 32u > 94u) return ID_EV_BADBYTE;
                        if (!id_put(S, ID_ROW_STR + ctx, b - 31u)) return ID_EV_OVERFLOW;
                        ctx = b - 31u;
                    }
                    if (!id_put(S, ID_ROW_STR + ctx, 0u)) return ID_EV_OVERFLOW;
                }
            }
            ci += ct; pi += pt; t++;
        }
        if (!id_put(S, id_min(t, 15u), ID_OP_END)) return ID_EV_OVERFLOW;
        prev = cur; plen = clen; at += clen + 1u;
    }
    return S.n;
}

// ---------------------------------------------------------------------------------------------------------------- the coder over a strand
// the nev events at ev, last to first, into [slab_lo, slab_hi) downwards from slab_hi.  -> its bytes (they end at slab_hi), 0 without events,
// QV_SLAB_OVERFLOW when the slab is too small or an event has no frequency (never)
QV_HD uint32_t id_strand_encode(const uint16_t *ev, uint32_t nev, const uint32_t *fc, uint8_t *slab_lo, uint8_t *slab_hi)
{
    if (!nev) return 0;
    uint32_t x = QV_LOW; uint8_t *p = slab_hi;
    for (uint32_t k = nev; k-- > 0;) {
        const uint32_t v = ev[k], e = fc[id_row_off(v >> 8) + (v & 255u)];
        if (p - slab_lo < 6 || !(e & 0xFFFFu)) return QV_SLAB_OVERFLOW;
        qv_enc_step(x, e, p);
    }
    p -= 4;
    p[0] = (uint8_t)(x >> 24); p[1] = (uint8_t)(x >> 16); p[2] = (uint8_t)(x >> 8); p[3] = (uint8_t)x;
    return (uint32_t)(slab_hi - p);
}
QV_HD int id_dec(uint32_t &x, const uint32_t *fc, uint32_t row, const uint8_t *&p, const uint8_t *end, uint32_t *y)
{
    return qv_dec_step(x, fc + id_row_off(row), id_row_width(row), p, end, y);
}
// ... and back: the len bytes at src -> the nl lines of the strand, exactly tbytes bytes at out.  Every op writes at least one byte and every line its newline,
// and no byte is written at or behind out + tbytes: the walk ends whatever the bytes at src are
QV_HD int id_strand_decode(const uint8_t *src, uint32_t len, const uint32_t *fc, uint8_t *out, uint32_t tbytes, uint32_t nl)
{
    if (!nl) return (len || tbytes) ? ID_E_SHORT : ID_OK;
    if (len < 4u || tbytes < nl) return ID_E_SHORT;
    const uint8_t *p = src + 4, *end = src + len;
    uint32_t x = ((uint32_t)src[0] << 24) | ((uint32_t)src[1] << 16) | ((uint32_t)src[2] << 8) | (uint32_t)src[3];
    if (x < QV_LOW) return ID_E_END;
    uint32_t w = 0, prev_at = 0, plen = 0;
    for (uint32_t i = 0; i < nl; i++) {
        const uint32_t cur_at = w;
        uint32_t pi = 0, t = 0;
        for (;;) {
            uint32_t op;
            int e = id_dec(x, fc, id_min(t, 15u), p, end, &op);
            if (e) return e;
            if (op == ID_OP_END) break;
            const uint32_t hp = pi < plen, pt = hp ? id_tok_len(out + prev_at + pi, plen - pi) : 0u;
            if (op == ID_OP_MATCH) {
                if (!hp) return ID_E_PREV;
                if (tbytes - w < pt) return ID_E_TEXT;
                for (uint32_t k = 0; k < pt; k++) out[w + k] = out[prev_at + pi + k];
                w += pt;
            } else if (op == ID_OP_STR) {
                uint32_t ctx = 0;
                for (;;) {
                    uint32_t y;
                    e = id_dec(x, fc, ID_ROW_STR + ctx, p, end, &y);
                    if (e) return e;
                    if (!y) break;
                    if (w >= tbytes) return ID_E_TEXT;
                    out[w++] = (uint8_t)(y + 31u);
                    ctx = y;
                }
                if (!ctx) return ID_E_EMPTY;
            } else {
                uint32_t v = 0;
                if (op == ID_OP_DELTA) {
                    const uint32_t pv = hp ? id_tok_value(out + prev_at + pi, pt) : ID_NOT_NUMERIC;
                    if (pv == ID_NOT_NUMERIC) return ID_E_PREV;
                    uint32_t d;
                    e = id_dec(x, fc, ID_ROW_DELTA + id_min(t, 7u), p, end, &d);
                    if (e) return e;
                    if (!d) return ID_E_VALUE;
                    v = pv + d;
                } else {
                    for (uint32_t k = 0; k < 4u; k++) {
                        uint32_t y;
                        e = id_dec(x, fc, ID_ROW_NUM + k, p, end, &y);
                        if (e) return e;
                        v |= y << (8u * k);
                    }
                }
                if (v > ID_MAX_VALUE) return ID_E_VALUE;
                uint32_t nd = 1, div = 1;
                while (v / div >= 10u) { div *= 10u; nd++; }
                if (tbytes - w < nd) return ID_E_TEXT;
                for (; div; div /= 10u) out[w++] = (uint8_t)(48u + (v / div) % 10u);
            }
            pi += pt; t++;
        }
        if (w >= tbytes) return ID_E_TEXT;
        out[w++] = '\n';
        prev_at = cur_at; plen = w - 1u - cur_at;
    }
    if (w != tbytes) return ID_E_TEXT;
    return x == QV_LOW && p == end ? ID_OK : ID_E_END;
}

// ---------------------------------------------------------------------------------------------------------------- the table in the payload
QV_HD uint32_t id_bm_bit(const uint32_t *bm, uint32_t r) { return (bm[r >> 5] >> (r & 31u)) & 1u; }
// entries of the present rows in front of row r (r = ID_ROWS: of all of them)
QV_HD uint32_t id_rows_before(const uint32_t *bm, uint32_t r)
{
    uint32_t n = 0;
    for (uint32_t k = 0; k < r; k++) if (id_bm_bit(bm, k)) n += id_row_width(k);
    return n;
}
// Normalise row r of counts to 4096 and make it frequency | cumulative << 16; -> 1 when the row is present (it holds a count).  The rule is qv_norm_row's:
// f = max(1, floor(c * 4096 / T)), the difference to 4096 to the largest count.  Its argument that the largest count can pay holds for rows of at most 94
// symbols.  A row of 256 can hold more entries lifted to 1 than its largest frequency (39 common differences and 154 rare ones: 107 < 154): then the excess
// is taken from all entries in turn, in ascending symbol order, a sixteenth of each, then an eighth, a quarter and halves until it is gone.  f >> shift < f, so an entry stays
// >= 1; the sum is above 4096 >= 16 A, so some entry is >= 17 and every round takes something
// (id_norm_counts: the rule over any row of A <= 256 counts -- sv_block.h normalises its rows of 256 byte values with it)
QV_HD int id_norm_counts(uint32_t *row, uint32_t A)
{
    uint64_t T = 0; uint32_t best = 0;
    for (uint32_t y = 0; y < A; y++) { const uint32_t c = row[y]; T += c; if (c > best) best = c; }
    if (!T) return 0;
    uint32_t sum = 0;
    for (uint32_t y = 0; y < A; y++) { const uint32_t c = row[y]; if (c) { const uint32_t f = (uint32_t)(((uint64_t)c << 12) / T); sum += f ? f : 1u; } }
    uint32_t fb = (uint32_t)(((uint64_t)best << 12) / T);
    if (!fb) fb = 1;
    if (fb + QV_TOT > sum) qv_norm_row(row, A);
    else {
        for (uint32_t y = 0; y < A; y++) { const uint32_t c = row[y]; if (c) { const uint32_t f = (uint32_t)(((uint64_t)c << 12) / T); row[y] = f ? f : 1u; } }
        uint32_t excess = sum - QV_TOT;
        for (uint32_t shift = 4; excess; shift = shift > 1u ? shift - 1u : 1u)
            for (uint32_t y = 0; y < A && excess; y++) { const uint32_t d = id_min(excess, row[y] >> shift); row[y] -= d; excess -= d; }
    }
    qv_cum_row(row, A);
    return 1;
}
QV_HD int id_norm_row(uint32_t *fc, uint32_t r) { return id_norm_counts(fc + id_row_off(r), id_row_width(r)); }
// row r of the table at tab (the present rows, u16 frequencies) -> fc; an absent row is all zero: no slot of it belongs to a symbol
QV_HD int id_load_row(const uint8_t *tab, const uint32_t *bm, uint32_t r, uint32_t *fc)
{
    uint32_t *row = fc + id_row_off(r);
    const uint32_t A = id_row_width(r);
    if (!id_bm_bit(bm, r)) { for (uint32_t y = 0; y < A; y++) row[y] = 0; return ID_OK; }
    if (qv_load_row(tab + 2u * id_rows_before(bm, r), 0, A, row)) return ID_E_ROW;
    return (row[A - 1u] >> 16) + (row[A - 1u] & 0xFFFFu) == QV_TOT ? ID_OK : ID_E_ROW;
}
// The prefix of a block, u32 payload_bytes and the mode and block_text_bytes that every payload starts with, at q with `left` bytes of the packed form from q on
// (fewer than ID_PREFIX: none of q is read) and text_left bytes of the text not yet claimed by the blocks in front: -> 1 with the size of a payload that holds its head
// and fits what is left behind the u32, and text bytes within the bound of a block and within text_left, or 0
#define ID_PREFIX (4u + ID_HEAD0)
QV_HD int id_prefix(const uint8_t *q, uint64_t left, uint64_t text_left, uint64_t *payload_bytes, uint64_t *text_bytes)
{
    if (left < ID_PREFIX) return 0;
    *payload_bytes = qv_le32(q); *text_bytes = qv_le32(q + 5);
    return *payload_bytes >= ID_HEAD0 && *payload_bytes <= left - 4u && *text_bytes <= ID_MAX_BLOCK_TEXT && *text_bytes <= text_left;
}
// the head of a payload of pbytes bytes: -> ID_OK with *mode and *tbytes, and for mode 1 bm[4] and *hdr1, the bytes in front of the strands
QV_HD int id_check_head(const uint8_t *pl, uint32_t pbytes, uint32_t *mode, uint32_t *tbytes, uint32_t *bm, uint32_t *hdr1)
{
    if (pbytes < ID_HEAD0) return ID_E_SIZE;
    *mode = pl[0]; *tbytes = qv_le32(pl + 1);
    if (*tbytes > ID_MAX_BLOCK_TEXT) return ID_E_SIZE;
    if (pl[0] == 0) return pbytes - ID_HEAD0 == *tbytes ? ID_OK : ID_E_SIZE;
    if (pl[0] != 1) return ID_E_MODE;
    if (pbytes < ID_HEAD1) return ID_E_SIZE;
    for (uint32_t k = 0; k < 4u; k++) bm[k] = qv_le32(pl + ID_HEAD1 - 16u + 4u * k);
    if (bm[3] >> (ID_ROWS - 96u)) return ID_E_BITMAP;
    *hdr1 = ID_HEAD1 + 2u * id_rows_before(bm, ID_ROWS);
    return pbytes < *hdr1 ? ID_E_SIZE : ID_OK;
}
// strand s of a coded payload for m lines: its text bytes and coded bytes as the head announces them
QV_HD int id_check_strand(const uint8_t *pl, uint32_t m, uint32_t s, uint32_t *stext, uint32_t *slen)
{
    *stext = qv_le32(pl + ID_HEAD0 + 4u * s); *slen = qv_le32(pl + ID_HEAD0 + 4u * ID_STRANDS + 4u * s);
    const uint32_t nl = id_strand_lines(m, s);
    if (nl ? (*slen < 4u || *stext < nl) : (*slen || *stext)) return ID_E_SHORT;
    return ID_OK;
}
QV_HD int id_use_coded(uint32_t hdr1, uint32_t strand_bytes, uint32_t tbytes) { return (uint64_t)hdr1 + strand_bytes < (uint64_t)ID_HEAD0 + tbytes; }
// a stored block of m lines: tbytes bytes with m newlines, the last byte one of them
QV_HD int id_stored_ok(const uint8_t *tx, uint32_t tbytes, uint32_t m)
{
    uint32_t nl = 0;
    for (uint32_t i = 0; i < tbytes; i++) nl += tx[i] == '\n';
    return nl == m && (!tbytes || tx[tbytes - 1u] == '\n');
}

// ---------------------------------------------------------------------------------------------------------------- one block on the host, in a row
struct IdWork {
    uint32_t fc[ID_TABLE];
    uint32_t bm[4];
    uint32_t soff[ID_STRANDS + 1], len[ID_STRANDS], nev[ID_STRANDS];
};
// what a caller must hand to id_block_encode for a block of tbytes bytes in m lines: u16 events, bytes of slabs
QV_HD uint64_t id_block_events(uint32_t tbytes, uint32_t m) { return (uint64_t)tbytes + 2ull * m; }
QV_HD uint64_t id_block_slabs(uint32_t tbytes, uint32_t m) { return 2ull * id_block_events(tbytes, m) + 32ull * ID_STRANDS; }

// the m lines in the tbytes bytes at text -> u32 payload_bytes and the payload at out.  -> the bytes of the block (9 + tbytes at most), 0 when cap is smaller
// (nothing is written then) or a slab overflowed (never).  *stored: the mode was 0
QV_HD uint32_t id_block_encode(const uint8_t *text, uint32_t tbytes, uint32_t m, IdWork &W, uint16_t *events, uint8_t *slabs, uint8_t *out, uint64_t cap, int *stored)
{
    const uint32_t stored_bytes = 4u + ID_HEAD0 + tbytes;
    {   // where the strands start
        uint32_t line = 0, s = 0;
        while (s < ID_STRANDS && id_strand_line0(m, s) == 0) W.soff[s++] = 0;
        for (uint32_t i = 0; i < tbytes; i++)
            if (text[i] == '\n') { line++; while (s < ID_STRANDS && id_strand_line0(m, s) == line) W.soff[s++] = i + 1u; }
        while (s <= ID_STRANDS) W.soff[s++] = tbytes;
    }
    for (uint32_t i = 0; i < ID_TABLE; i++) W.fc[i] = 0;
    int coded = 1; uint32_t total = 0, hdr1 = 0;
    for (uint32_t s = 0; s < ID_STRANDS; s++) {
        const uint32_t nl = id_strand_lines(m, s), tb = W.soff[s + 1] - W.soff[s];
        const uint32_t n = id_strand_events(text + W.soff[s], tb, nl, events + W.soff[s] + 2u * id_strand_line0(m, s), id_event_cap(tb, nl), W.fc);
        if (n == ID_EV_OVERFLOW || n == ID_EV_BADBYTE) { coded = 0; break; }
        W.nev[s] = n;
    }
    if (coded) {
        W.bm[0] = W.bm[1] = W.bm[2] = W.bm[3] = 0;
        for (uint32_t r = 0; r < ID_ROWS; r++) if (id_norm_row(W.fc, r)) W.bm[r >> 5] |= 1u << (r & 31u);
        for (uint32_t s = 0; s < ID_STRANDS; s++) {
            const uint32_t nl = id_strand_lines(m, s), tb = W.soff[s + 1] - W.soff[s], l0 = id_strand_line0(m, s);
            uint8_t *lo = slabs + 2ull * (W.soff[s] + 2u * l0) + 32u * s;
            const uint32_t n = id_strand_encode(events + W.soff[s] + 2u * l0, W.nev[s], W.fc, lo, lo + id_slab_bytes(id_event_cap(tb, nl)));
            if (n == QV_SLAB_OVERFLOW) return 0;
            W.len[s] = n; total += n;
        }
        hdr1 = ID_HEAD1 + 2u * id_rows_before(W.bm, ID_ROWS);
        coded = id_use_coded(hdr1, total, tbytes);
    }
    if (stored) *stored = !coded;
    if (!coded) {
        if (cap < stored_bytes) return 0;
        qv_put32(out, stored_bytes - 4u);
        out[4] = 0; qv_put32(out + 5, tbytes);
        for (uint32_t i = 0; i < tbytes; i++) out[9u + i] = text[i];
        return stored_bytes;
    }
    const uint32_t size = 4u + hdr1 + total;
    if (cap < size) return 0;
    qv_put32(out, size - 4u);
    uint8_t *o = out + 4;
    o[0] = 1; qv_put32(o + 1, tbytes);
    for (uint32_t s = 0; s < ID_STRANDS; s++) { qv_put32(o + ID_HEAD0 + 4u * s, W.soff[s + 1] - W.soff[s]); qv_put32(o + ID_HEAD0 + 4u * ID_STRANDS + 4u * s, W.len[s]); }
    for (uint32_t k = 0; k < 4u; k++) qv_put32(o + ID_HEAD1 - 16u + 4u * k, W.bm[k]);
    o += ID_HEAD1;
    for (uint32_t r = 0; r < ID_ROWS; r++) {
        if (!id_bm_bit(W.bm, r)) continue;
        const uint32_t *row = W.fc + id_row_off(r);
        for (uint32_t y = 0; y < id_row_width(r); y++) { const uint32_t f = row[y] & 0xFFFFu; *o++ = (uint8_t)f; *o++ = (uint8_t)(f >> 8); }
    }
    for (uint32_t s = 0; s < ID_STRANDS; s++) {
        const uint32_t nl = id_strand_lines(m, s), tb = W.soff[s + 1] - W.soff[s];
        const uint8_t *src = slabs + 2ull * (W.soff[s] + 2u * id_strand_line0(m, s)) + 32u * s + id_slab_bytes(id_event_cap(tb, nl)) - W.len[s];
        for (uint32_t i = 0; i < W.len[s]; i++) *o++ = src[i];
    }
    return size;
}

// the payload of a block of m lines (pbytes bytes, behind its u32) -> its text, tbytes bytes as the caller read them from the payload's head, at text.
// Reads only the payload, writes only the tbytes bytes
QV_HD int id_block_decode(const uint8_t *pl, uint32_t pbytes, uint32_t m, IdWork &W, uint8_t *text)
{
    uint32_t mode = 0, tbytes = 0, hdr1 = 0;
    const int e = id_check_head(pl, pbytes, &mode, &tbytes, W.bm, &hdr1);
    if (e) return e;
    if (mode == 0) {
        if (!id_stored_ok(pl + ID_HEAD0, tbytes, m)) return ID_E_TEXT;
        for (uint32_t i = 0; i < tbytes; i++) text[i] = pl[ID_HEAD0 + i];
        return ID_OK;
    }
    // every row and every strand is looked at, and the smallest code of what is wrong is the answer: the lanes of a workgroup agree on it in any order
    uint32_t bad = ID_E_NONE;
    for (uint32_t r = 0; r < ID_ROWS; r++) bad = id_min(bad, id_code(id_load_row(pl + ID_HEAD1, W.bm, r, W.fc)));
    uint64_t tsum = 0, lsum = 0;
    for (uint32_t s = 0; s < ID_STRANDS; s++) {
        uint32_t st, sl;
        bad = id_min(bad, id_code(id_check_strand(pl, m, s, &st, &sl)));
        tsum += st; lsum += sl;
    }
    if (tsum != tbytes) bad = id_min(bad, ID_E_SIZE);
    if (lsum != pbytes - hdr1) bad = id_min(bad, ID_E_LENGTHS);
    if (bad != ID_E_NONE) return (int)bad;
    const uint8_t *src = pl + hdr1;
    uint32_t tat = 0;
    for (uint32_t s = 0; s < ID_STRANDS; s++) {
        const uint32_t st = qv_le32(pl + ID_HEAD0 + 4u * s), sl = qv_le32(pl + ID_HEAD0 + 4u * ID_STRANDS + 4u * s);
        bad = id_min(bad, id_code(id_strand_decode(src, sl, W.fc, text + tat, st, id_strand_lines(m, s))));
        src += sl; tat += st;
    }
    return bad == ID_E_NONE ? ID_OK : (int)bad;
}
