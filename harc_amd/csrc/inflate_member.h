// inflate_member.h -- one BGZF member (SAM/BAM specification 4.1: a gzip member whose extra field carries a BC subfield) -> its text.
// The header walk, the code tables (RFC 1951 3.2.7: canonical codes kept as counts per length + symbols in code order), the symbol loop
// and every bounds check live here once: bgzf.hip runs them on the device, tests/test_bgzf_host.py builds this file with g++ and
// sanitizers and fuzzes it against zlib.  Safe for any input by construction: a member's decoder reads only inside its own CDATA
// (refills stop at its end), writes only inside its own ISIZE span and its own tables, rejects over-subscribed and incomplete
// code-length sets before a single lookup, and every loop is bounded by the bytes of CDATA or by ISIZE.
// No local arrays: on the device they would live in private memory.  The base / extra-bit tables of RFC 1951 3.2.5 are computed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IM_HD __host__ __device__ __forceinline__
#else
#define IM_HD static inline
#endif

// result codes (0 = the member decoded to exactly ISIZE bytes with the trailer's CRC-32)
enum {
    IM_OK = 0,
    IM_E_TRUNC = 1,        // the DEFLATE stream needs bits beyond the end of CDATA
    IM_E_BTYPE = 2,        // block type 3
    IM_E_STORED = 3,       // stored block: LEN / NLEN disagree
    IM_E_CODES = 4,        // code-length set over-subscribed, incomplete, or without an end-of-block code
    IM_E_SYMBOL = 5,       // a bit pattern that no code of the block decodes, or length / distance symbols 286-287 / 30-31
    IM_E_DIST = 6,         // a distance that reaches before the member's first byte
    IM_E_OVERFLOW = 7,     // more text than ISIZE
    IM_E_SHORT = 8,        // less text than ISIZE
    IM_E_CRC = 9,          // CRC-32 of the text differs from the trailer
    IM_E_HEADER = 10,      // no BGZF header at the member's offset
    IM_E_ISIZE = 11,       // ISIZE > 65536
    IM_E_GZHEADER = 12,    // inflate_stream.h: no RFC 1952 member header (magic, CM other than 8, a reserved flag bit)
    IM_E_TRAILING = 13,    // inflate_stream.h: bytes behind a member's trailer that are no member header
    IM_E_LENGTH = 14,      // inflate_stream.h: the text's length mod 2^32 differs from the trailer's ISIZE
};

#define IM_MAXBITS 15
#define IM_NLIT 288
#define IM_NDIST 32

// the tables of one block: counts of codes per length, symbols ordered by code (what im_decode walks), the code lengths being read
struct ImTables {
    uint16_t lcount[IM_MAXBITS + 1];
    uint16_t lsym[IM_NLIT];
    uint16_t dcount[IM_MAXBITS + 1];
    uint16_t dsym[IM_NDIST];
    uint16_t offs[IM_MAXBITS + 1];
    uint8_t len[IM_NLIT + IM_NDIST];
};
// ---------------------------------------------------------------------------------------------------------------- gzip / BGZF header
// A BGZF member header at p (avail bytes readable there): 1f 8b 08, FEXTRA, a BC subfield of two bytes anywhere in the extra field.
// -> 1 with *bsize (= member size - 1) and *hdr (bytes in front of CDATA = 12 + XLEN), 0 otherwise.  The header must leave room for the
// 8-byte trailer inside BSIZE + 1; nothing at or past p + avail is read.
IM_HD int im_bgzf_header(const uint8_t *p, uint64_t avail, uint32_t *bsize, uint32_t *hdr)
{
    if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const uint32_t xlen = (uint32_t)p[10] | ((uint32_t)p[11] << 8);
    if (12ull + xlen > avail) return 0;
    int found = 0; uint32_t bs = 0;
    for (uint32_t k = 0; k + 4 <= xlen;) {                 // subfields: SI1 SI2 SLEN(2) data
        const uint8_t *s = p + 12 + k;
        const uint32_t slen = (uint32_t)s[2] | ((uint32_t)s[3] << 8);
        if (k + 4 + slen > xlen) return 0;
        if (s[0] == 'B' && s[1] == 'C' && slen == 2 && !found) { bs = (uint32_t)s[4] | ((uint32_t)s[5] << 8); found = 1; }
        k += 4 + slen;
    }
    if (!found || bs + 1 < 12 + xlen + 8) return 0;
    *bsize = bs; *hdr = 12 + xlen;
    return 1;
}
IM_HD uint32_t im_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---------------------------------------------------------------------------------------------------------------- bit reader
struct ImBits {
    const uint8_t *in; uint32_t n, pos;     // CDATA and the next byte to take
    uint32_t buf; int cnt;                  // bits not yet consumed, LSB first
};
// at least `need` (<= 16) bits in the buffer; refills stop at the end of CDATA
IM_HD int im_need(ImBits &b, int need)
{
    while (b.cnt < need) {
        if (b.pos >= b.n) return IM_E_TRUNC;
        b.buf |= (uint32_t)b.in[b.pos++] << b.cnt;
        b.cnt += 8;
    }
    return IM_OK;
}
IM_HD uint32_t im_take(ImBits &b, int k)
{
    const uint32_t v = b.buf & ((1u << k) - 1u);
    b.buf >>= k; b.cnt -= k;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- code tables
// canonical code from the lengths len[0 .. n): counts per length and symbols in code order.  -> the code space left (0 = complete,
// > 0 = incomplete), < 0 when over-subscribed.  No table is looked up here.
IM_HD int im_build(const uint8_t *len, int n, uint16_t *count, uint16_t *sym, uint16_t *offs)
{
    for (int l = 0; l <= IM_MAXBITS; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[len[s]]++;
    if (count[0] == n) return 1;                           // no codes at all: incomplete, and no symbol decodes
    int left = 1;
    for (int l = 1; l <= IM_MAXBITS; l++) {
        left <<= 1; left -= count[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int l = 1; l < IM_MAXBITS; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; s++) if (len[s]) sym[offs[len[s]]++] = (uint16_t)s;
    return left;
}
// one symbol: the canonical code read bit by bit (the code's first bit first), at most 15 steps.  On a table that im_build did not reject
// the index stays below the number of symbols that have a length.
IM_HD int im_decode(ImBits &b, const uint16_t *count, const uint16_t *sym, int *out)
{
    int code = 0, first = 0, index = 0;
    uint32_t buf = b.buf; int cnt = b.cnt;
    for (int l = 1; l <= IM_MAXBITS; l++) {
        if (cnt == 0) {
            if (b.pos >= b.n) return IM_E_TRUNC;
            buf = b.in[b.pos++]; cnt = 8;
        }
        code |= (int)(buf & 1u); buf >>= 1; cnt--;
        const int c = count[l];
        if (code - c < first) { b.buf = buf; b.cnt = cnt; *out = sym[index + (code - first)]; return IM_OK; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return IM_E_SYMBOL;
}

// ---------------------------------------------------------------------------------------------------------------- CRC-32 (gzip)
IM_HD uint32_t im_crc_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

// ---------------------------------------------------------------------------------------------------------------- one member
// RFC 1951 3.2.5: length symbol 257 + s (s < 29) and distance symbol d (d < 30) -> extra bits and base
IM_HD int im_lext(int s) { return (s < 8 || s == 28) ? 0 : (s - 4) >> 2; }
IM_HD uint32_t im_lbase(int s) { return s < 8 ? 3u + (uint32_t)s : s == 28 ? 258u : ((4u + (uint32_t)(s & 3)) << im_lext(s)) + 3u; }
IM_HD int im_dext(int d) { return d < 4 ? 0 : (d - 2) >> 1; }
IM_HD uint32_t im_dbase(int d) { return d < 4 ? 1u + (uint32_t)d : ((2u + (uint32_t)(d & 1)) << im_dext(d)) + 1u; }
// order in which the code-length code lengths arrive (RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15), 5 bits each
IM_HD int im_clorder(int k)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45;
    const uint64_t hi = 11ull | 4ull << 5 | 12ull << 10 | 3ull << 15 | 13ull << 20 | 2ull << 25 | 14ull << 30 | 1ull << 35 | 15ull << 40;
    return (int)(((k < 10 ? lo >> (5 * k) : hi >> (5 * (k - 10)))) & 31u);
}
// The symbols of one Huffman block into out[*at .. cap).  Every literal or match writes at least one byte below cap, so the loop ends
// within cap symbols plus the end-of-block code (or at the end of CDATA).
IM_HD int im_codes(ImBits &b, const ImTables &t, uint8_t *out, uint32_t *at, uint32_t cap)
{
    uint32_t o = *at;
    for (;;) {
        int s; int rc = im_decode(b, t.lcount, t.lsym, &s);
        if (rc) return rc;
        if (s < 256) {
            if (o >= cap) return IM_E_OVERFLOW;
            out[o++] = (uint8_t)s;
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
        const uint32_t dist = im_dbase(ds) + im_take(b, de);
        if (dist > o) return IM_E_DIST;
        if (len > cap - o) return IM_E_OVERFLOW;
        const uint8_t *src = out + (o - dist);
        for (uint32_t k = 0; k < len; k++) out[o + k] = src[k];           // byte by byte: dist < len replicates the period
        o += len;
    }
    *at = o;
    return IM_OK;
}
IM_HD void im_fixed(ImTables &t)
{
    int s = 0;
    for (; s < 144; s++) t.len[s] = 8;
    for (; s < 256; s++) t.len[s] = 9;
    for (; s < 280; s++) t.len[s] = 7;
    for (; s < IM_NLIT; s++) t.len[s] = 8;
    (void)im_build(t.len, IM_NLIT, t.lcount, t.lsym, t.offs);        // complete
    for (s = 0; s < 30; s++) t.len[s] = 5;
    (void)im_build(t.len, 30, t.dcount, t.dsym, t.offs);             // incomplete on purpose: codes 30 and 31 do not decode
}
IM_HD int im_dynamic(ImBits &b, ImTables &t)
{
    int rc;
    if ((rc = im_need(b, 14))) return rc;
    const int nlen = (int)im_take(b, 5) + 257, ndist = (int)im_take(b, 5) + 1, ncode = (int)im_take(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return IM_E_CODES;
    int k = 0;
    for (; k < ncode; k++) { if ((rc = im_need(b, 3))) return rc; t.len[im_clorder(k)] = (uint8_t)im_take(b, 3); }
    for (; k < 19; k++) t.len[im_clorder(k)] = 0;
    if (im_build(t.len, 19, t.lcount, t.lsym, t.offs) != 0) return IM_E_CODES;       // the code-length code must be complete
    for (k = 0; k < nlen + ndist;) {
        int s; if ((rc = im_decode(b, t.lcount, t.lsym, &s))) return rc;
        if (s < 16) { t.len[k++] = (uint8_t)s; continue; }
        uint8_t v = 0; int rep;
        if (s == 16) {
            if (k == 0) return IM_E_CODES;                     // nothing to repeat
            v = t.len[k - 1];
            if ((rc = im_need(b, 2))) return rc;
            rep = 3 + (int)im_take(b, 2);
        } else if (s == 17) { if ((rc = im_need(b, 3))) return rc; rep = 3 + (int)im_take(b, 3); }
        else { if ((rc = im_need(b, 7))) return rc; rep = 11 + (int)im_take(b, 7); }
        if (k + rep > nlen + ndist) return IM_E_CODES;
        while (rep--) t.len[k++] = v;
    }
    if (t.len[256] == 0) return IM_E_CODES;                 // no end-of-block code
    // an incomplete code is allowed only as a single code of one bit (RFC 1951 3.2.7; zlib's rule), and a block may have no distance codes
    // at all (it holds literals only: decoding a distance then fails, the counts are all zero)
    int left = im_build(t.len, nlen, t.lcount, t.lsym, t.offs);
    if (left < 0 || (left > 0 && !(nlen - t.lcount[0] == 1 && t.lcount[1] == 1))) return IM_E_CODES;
    left = im_build(t.len + nlen, ndist, t.dcount, t.dsym, t.offs);
    if (left < 0 || (left > 0 && ndist - t.dcount[0] != 0 && !(ndist - t.dcount[0] == 1 && t.dcount[1] == 1))) return IM_E_CODES;
    return IM_OK;
}
// The DEFLATE stream cdata[0 .. n) -> out[0 .. isize), then the CRC-32 of that text against `crc`.  t: the caller's tables (device: this
// lane's slot in global memory; host: the stack).  crctab: im_crc_entry(0 .. 255).
IM_HD int im_inflate(const uint8_t *cdata, uint32_t n, uint8_t *out, uint32_t isize, uint32_t crc, ImTables &t, const uint32_t *crctab)
{
    ImBits b; b.in = cdata; b.n = n; b.pos = 0; b.buf = 0; b.cnt = 0;
    uint32_t o = 0; int last = 0, rc;
    do {
        if ((rc = im_need(b, 3))) return rc;
        last = (int)im_take(b, 1);
        const int type = (int)im_take(b, 2);
        if (type == 0) {
            b.buf = 0; b.cnt = 0;                              // the rest of the current byte is dropped
            if (b.n - b.pos < 4) return IM_E_TRUNC;
            const uint32_t len = (uint32_t)b.in[b.pos] | ((uint32_t)b.in[b.pos + 1] << 8), nlen = (uint32_t)b.in[b.pos + 2] | ((uint32_t)b.in[b.pos + 3] << 8);
            b.pos += 4;
            if (len != (~nlen & 0xFFFFu)) return IM_E_STORED;
            if (len > b.n - b.pos) return IM_E_TRUNC;
            if (len > isize - o) return IM_E_OVERFLOW;
            for (uint32_t k = 0; k < len; k++) out[o + k] = b.in[b.pos + k];
            b.pos += len; o += len;
        } else if (type == 1) {
            im_fixed(t);
            if ((rc = im_codes(b, t, out, &o, isize))) return rc;
        } else if (type == 2) {
            if ((rc = im_dynamic(b, t))) return rc;
            if ((rc = im_codes(b, t, out, &o, isize))) return rc;
        } else return IM_E_BTYPE;
    } while (!last);
    if (o != isize) return IM_E_SHORT;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < isize; k++) c = crctab[(c ^ out[k]) & 0xFFu] ^ (c >> 8);
    if ((c ^ 0xFFFFFFFFu) != crc) return IM_E_CRC;
    return IM_OK;
}
// A whole member at p (avail bytes readable there) into out[0 .. out_cap): header, CDATA, trailer.  -> IM_OK with *member_bytes and
// *text_bytes, or an IM_E_* code.  The host test's entry point; the device parses the header in k_bgzf_cand_* and calls im_inflate.
IM_HD int im_member(const uint8_t *p, uint64_t avail, uint8_t *out, uint32_t out_cap, ImTables &t, const uint32_t *crctab, uint32_t *member_bytes, uint32_t *text_bytes)
{
    uint32_t bsize = 0, hdr = 0;
    if (!im_bgzf_header(p, avail, &bsize, &hdr)) return IM_E_HEADER;
    if ((uint64_t)bsize + 1 > avail) return IM_E_TRUNC;
    const uint32_t crc = im_le32(p + bsize + 1 - 8), isize = im_le32(p + bsize + 1 - 4);
    if (isize > 65536) return IM_E_ISIZE;
    if (isize > out_cap) return IM_E_OVERFLOW;
    *member_bytes = bsize + 1; *text_bytes = isize;
    return im_inflate(p + hdr, bsize + 1 - hdr - 8, out, isize, crc, t, crctab);
}
