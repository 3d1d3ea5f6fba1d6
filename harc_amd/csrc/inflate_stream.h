// inflate_stream.h -- a gzip member of any size (RFC 1952 around one RFC 1951 stream) inflated in parallel, the way pugz and rapidgzip do it on CPUs: the
// compressed bytes are cut into chunks, in every chunk the first bit offset at which a non-final dynamic block header parses is a candidate start
// (is_find), a walk decodes block after block from its start to the first block boundary behind its chunk (is_walk; once only counting, once writing),
// and what a walk cannot know -- the 32 KiB of text in front of its first byte -- stays symbolic: a walk writes 16-bit symbols, a literal as 0..255, a
// byte of the unknown window as 0x8000 | index.  The windows are then resolved in file order (is_window_byte) and the symbols translated (is_translate).
// gunzip.hip runs all of it on the device and, in a row, on the host; tests/test_gunzip_host.py builds this file with g++ and sanitizers.
// The bit reader, the code tables, im_dynamic, im_fixed and the base / extra-bit functions are inflate_member.h's.  No local arrays.  Every loop is bounded
// by the compressed bytes it was given (a symbol takes at least one bit) or by the capacity of its output.
#pragma once
#include "inflate_member.h"

#define IS_WIN 32768u
#define IS_NONE (~0ull)

// ---------------------------------------------------------------------------------------------------------------- gzip header
// Any RFC 1952 member header at p (avail bytes readable there): FEXTRA, FNAME, FCOMMENT, FHCRC, any MTIME / XFL / OS.  -> IM_OK with *hdr_bytes (the
// DEFLATE stream starts there), IM_E_TRUNC when the header runs past avail, IM_E_GZHEADER for anything else: no magic, CM other than 8, a reserved flag bit.
IM_HD int gz_header(const uint8_t *p, uint64_t avail, uint64_t *hdr_bytes)
{
    if (avail >= 1 && p[0] != 0x1f) return IM_E_GZHEADER;
    if (avail >= 2 && p[1] != 0x8b) return IM_E_GZHEADER;
    if (avail >= 3 && p[2] != 8) return IM_E_GZHEADER;
    if (avail >= 4 && (p[3] & 0xE0)) return IM_E_GZHEADER;
    if (avail < 10) return IM_E_TRUNC;
    const int flg = p[3];
    uint64_t at = 10;
    if (flg & 4) {
        if (at + 2 > avail) return IM_E_TRUNC;
        at += 2 + ((uint64_t)p[at] | ((uint64_t)p[at + 1] << 8));
        if (at > avail) return IM_E_TRUNC;
    }
    for (int f = 8; f <= 16; f <<= 1)                      // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            for (;;) {
                if (at >= avail) return IM_E_TRUNC;
                if (p[at++] == 0) break;
            }
        }
    if (flg & 2) { at += 2; if (at > avail) return IM_E_TRUNC; }
    *hdr_bytes = at;
    return IM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- a bit offset of a long input
// The reader of inflate_member.h counts bytes in 32 bits: it is based at the byte that holds `bit`, and sees at most 2^32 - 16 bytes from there.
IM_HD int is_open(ImBits &b, const uint8_t *data, uint64_t n_bytes, uint64_t bit)
{
    const uint64_t byte0 = bit >> 3, rest = byte0 < n_bytes ? n_bytes - byte0 : 0;
    b.in = data + (byte0 < n_bytes ? byte0 : n_bytes); b.n = rest > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)rest; b.pos = 0; b.buf = 0; b.cnt = 0;
    const int skip = (int)(bit & 7u);
    if (skip) { const int rc = im_need(b, skip); if (rc) return rc; (void)im_take(b, skip); }
    return IM_OK;
}
IM_HD uint64_t is_tell(const ImBits &b, uint64_t bit0) { return ((bit0 >> 3) << 3) + (uint64_t)b.pos * 8u - (uint64_t)b.cnt; }

// ---------------------------------------------------------------------------------------------------------------- finder
// 1 when a non-final dynamic block header parses at `bit`: BFINAL = 0, BTYPE = 2, then HLIT <= 29 and HDIST <= 29 from the same four bytes before any
// table is built, then every check of im_dynamic.  Stored, fixed and final blocks are never candidates.
IM_HD int is_try(const uint8_t *data, uint64_t n_bytes, uint64_t bit, ImTables &t)
{
    const uint64_t byte0 = bit >> 3;
    if (byte0 + 4 > n_bytes) return 0;                     // 17 bits of header and at least one code length: nothing that short is a block
    const uint32_t v = im_le32(data + byte0) >> (bit & 7u);
    if ((v & 7u) != 4u) return 0;
    if (((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) return 0;
    ImBits b;
    if (is_open(b, data, n_bytes, bit) || im_need(b, 3)) return 0;
    (void)im_take(b, 3);
    return im_dynamic(b, t) == IM_OK;
}
// the first such bit offset in [bit_lo, bit_hi), or IS_NONE
IM_HD uint64_t is_find(const uint8_t *data, uint64_t n_bytes, uint64_t bit_lo, uint64_t bit_hi, ImTables &t)
{
    for (uint64_t bit = bit_lo; bit < bit_hi; bit++) if (is_try(data, n_bytes, bit, t)) return bit;
    return IS_NONE;
}

// ---------------------------------------------------------------------------------------------------------------- a walk
// what a walk found: the block boundary where it stopped (after an error: the bit where the error showed), the text bytes up to there, whether the block in
// front of that boundary was a final one, and whether the walk stopped because it needs bytes behind the end of the input
struct IsWalk { uint64_t end_bit, text; int32_t final, more; };

// The symbols of one Huffman block; out == nullptr: counted only (a back-reference needs no window to be counted).  A copy takes symbols, so markers propagate;
// a distance that reaches before the walk's first byte gives 0x8000 | index into the 32 KiB in front of that byte.
IM_HD int is_codes(ImBits &b, const ImTables &t, uint16_t *out, uint64_t *at, uint64_t cap)
{
    uint64_t o = *at;
    for (;;) {
        int s; int rc = im_decode(b, t.lcount, t.lsym, &s);
        if (rc) return rc;
        if (s < 256) {
            if (out) { if (o >= cap) return IM_E_OVERFLOW; out[o] = (uint16_t)s; }
            o++;
            continue;
        }
        if (s == 256) break;
        s -= 257;
        if (s >= 29) return IM_E_SYMBOL;
        const int le = im_lext(s);
        if ((rc = im_need(b, le))) return rc;
        const uint32_t len = im_lbase(s) + im_take(b, le);
        int ds; if ((rc = im_decode(b, t.dcount, t.dsym, &ds))) return rc;
        if (ds >= 30) return IM_E_SYMBOL;
        const int de = im_dext(ds);
        if ((rc = im_need(b, de))) return rc;
        const uint32_t dist = im_dbase(ds) + im_take(b, de);          // at most 32 768
        if (out) {
            if (len > cap - o) return IM_E_OVERFLOW;
            for (uint32_t k = 0; k < len; k++) {
                const uint64_t p = o + k;
                out[p] = p >= dist ? out[p - dist] : (uint16_t)(0x8000u | (uint32_t)(IS_WIN + p - dist));
            }
        }
        o += len;
    }
    *at = o;
    return IM_OK;
}
// one block of any type
IM_HD int is_block(ImBits &b, ImTables &t, uint16_t *out, uint64_t *at, uint64_t cap, int *last)
{
    int rc;
    if ((rc = im_need(b, 3))) return rc;
    *last = (int)im_take(b, 1);
    const int type = (int)im_take(b, 2);
    if (type == 0) {
        b.buf = 0; b.cnt = 0;                              // the rest of the current byte is dropped
        if (b.n - b.pos < 4) return IM_E_TRUNC;
        const uint32_t len = (uint32_t)b.in[b.pos] | ((uint32_t)b.in[b.pos + 1] << 8), nlen = (uint32_t)b.in[b.pos + 2] | ((uint32_t)b.in[b.pos + 3] << 8);
        if (len != (~nlen & 0xFFFFu)) return IM_E_STORED;
        b.pos += 4;
        if (len > b.n - b.pos) return IM_E_TRUNC;
        if (out) {
            if (len > cap - *at) return IM_E_OVERFLOW;
            for (uint32_t k = 0; k < len; k++) out[*at + k] = b.in[b.pos + k];
        }
        b.pos += len; *at += len;
        return IM_OK;
    }
    if (type == 1) im_fixed(t);
    else if (type == 2) { if ((rc = im_dynamic(b, t))) return rc; }
    else return IM_E_BTYPE;
    return is_codes(b, t, out, at, cap);
}
// Block after block from `bit` to the first block boundary at or behind stop_bit, or behind a final block.  out == nullptr: the count pass; else the write
// pass into out[0 .. cap), the same walk (give it the count pass's end_bit as stop_bit and its text as cap).  A block that needs bytes behind the end of
// the input is no error: the walk ends at the boundary in front of it with r->more set.  Any other decode error is returned, with r->end_bit where it showed.
IM_HD int is_walk(const uint8_t *data, uint64_t n_bytes, uint64_t bit, uint64_t stop_bit, ImTables &t, uint16_t *out, uint64_t cap, IsWalk *r)
{
    r->end_bit = bit; r->text = 0; r->final = 0; r->more = 0;
    ImBits b;
    if (is_open(b, data, n_bytes, bit)) { r->more = 1; return IM_OK; }
    uint64_t o = 0, cur = bit;
    while (cur < stop_bit) {
        int last = 0;
        const int rc = is_block(b, t, out, &o, cap, &last);
        if (rc == IM_E_TRUNC) { r->more = 1; return IM_OK; }
        if (rc) { r->end_bit = is_tell(b, bit); return rc; }
        cur = is_tell(b, bit);
        r->end_bit = cur; r->text = o;
        if (last) { r->final = 1; break; }
    }
    return IM_OK;
}
IM_HD int is_count(const uint8_t *data, uint64_t n_bytes, uint64_t bit, uint64_t stop_bit, ImTables &t, IsWalk *r) { return is_walk(data, n_bytes, bit, stop_bit, t, nullptr, 0, r); }

// ---------------------------------------------------------------------------------------------------------------- window step
// A window is IS_WIN bytes, the text in front of a walk, its newest byte last; `have` of them exist (a member's window starts empty).
IM_HD uint8_t is_resolve(uint16_t s, const uint8_t *win) { return (s & 0x8000u) ? win[s & 0x7FFFu] : (uint8_t)s; }
// byte j of the window behind a walk of T symbols whose resolved incoming window is win
IM_HD uint8_t is_window_byte(const uint8_t *win, const uint16_t *sym, uint64_t T, uint32_t j)
{
    if (T >= IS_WIN) return is_resolve(sym[T - IS_WIN + j], win);
    return (uint64_t)j + T < IS_WIN ? win[j + T] : is_resolve(sym[j + T - IS_WIN], win);
}
IM_HD uint32_t is_window_have(uint32_t have, uint64_t T) { const uint64_t h = (uint64_t)have + T; return h > IS_WIN ? IS_WIN : (uint32_t)h; }
// one symbol -> its byte.  A marker below what exists reaches before the member's first byte
IM_HD int is_translate(uint16_t s, const uint8_t *win, uint32_t have, uint8_t *out)
{
    if (s & 0x8000u) {
        const uint32_t i = s & 0x7FFFu;
        if (i < IS_WIN - have) return IM_E_DIST;
        *out = win[i];
    } else *out = (uint8_t)s;
    return IM_OK;
}
