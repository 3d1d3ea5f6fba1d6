// deflate_member.h -- text -> one BGZF member (SAM/BAM specification 4.1), the counterpart of inflate_member.h.  Everything that decides a byte of a
// member lives here once: bgzf_out.hip runs it on the device (a workgroup per member, the walk over the text spread over its lanes), tests/test_bgzf_out_host.py
// builds this file with g++ and sanitizers and holds it to zlib.  The serial encoder at the end (dm_member) and the kernel apply the same rules through the
// same functions, so both write the same bytes.  No local arrays: every table is in the caller's DmCodes (device: LDS; host: the heap).
//
// TOKEN RULE.  No search: FASTQ repeats itself four lines up, at the same column.  A line starts at byte 0 of the member and behind every newline.  For a byte
// j of line k whose line k - 4 starts inside the member at distance D = start[k] - start[k - 4] <= 32 768, the byte is EQUAL when text[j] == text[j - D].  A
// maximal run of equal bytes with one D (it may cross a newline while D stays the same) of R >= 4 bytes becomes matches (length, D), every other byte a
// literal.  A run is cut into pieces by dm_piece: pieces of 258 from its front; a remainder of 1 or 2 is taken out of the last full piece (258 + r becomes
// 255 + r and 3), so no piece is shorter than 3 and none longer than 258.  Nothing refers to a byte in front of the member.
// BLOCK.  One dynamic Huffman block (RFC 1951 3.2.7) per member: code lengths from the two histograms by the minimum-redundancy construction of Moffat and
// Katajainen on the sorted counts, limited to 15 bits (7 for the code-length code) by moving codes down from the limit until the Kraft sum is 1 again; the
// code lengths run-length coded greedily (dm_rle).  A member whose dynamic block is not smaller than a stored block is written stored: 65 280 + 5 + 26 bytes.
// FRAME.  The 18-byte header with XLEN = 6 and the BC subfield alone, CDATA, CRC-32 (partial CRCs of 64-byte chunks combined by multiplication with
// x^(8 len) mod P, the way the kernel's lanes do it), ISIZE.  The text of a file is cut every 65 280 bytes (DM_TEXT, bgzip's size).
#pragma once
#include "inflate_member.h"

#define DM_TEXT 65280u                  // bytes of text per member
#define DM_MEMBER_MAX (DM_TEXT + 31u)   // a stored member: 18 + 5 + text + 8
#define DM_NLL 286
#define DM_ND 30
#define DM_NCL 19
#define DM_MINRUN 4u
#define DM_MAXDIST 32768u
#define DM_NONE 0xFFFFFFFFu
#define DM_CRC_CHUNK 64u

IM_HD int dm_log2(uint32_t v) { return 31 - __builtin_clz(v); }       // v > 0
// the inverse of im_lbase / im_dbase: length 3 .. 258 -> symbol 257 + s, distance 1 .. 32 768 -> symbol d
IM_HD int dm_lsym(uint32_t len)
{
    if (len < 11) return (int)len - 3;
    if (len == 258) return 28;
    const uint32_t v = len - 3; const int e = dm_log2(v) - 2;          // v in [4 << e, 8 << e)
    return 4 * e + 4 + (int)((v >> e) & 3u);
}
IM_HD int dm_dsym(uint32_t dist)
{
    if (dist < 5) return (int)dist - 1;
    const uint32_t v = dist - 1; const int e = dm_log2(v) - 1;         // v in [2 << e, 4 << e)
    return 2 * e + 2 + (int)((v >> e) & 1u);
}
// the distance of a line that starts at s0 when the line four back starts at s4 (DM_NONE: there is none); 0 = no match possible
IM_HD uint32_t dm_D(uint32_t s0, uint32_t s4) { return (s4 != DM_NONE && s0 - s4 <= DM_MAXDIST) ? s0 - s4 : 0u; }
// a run of R >= DM_MINRUN equal bytes: the length of the piece that starts at offset o of the run, 0 when none starts there
IM_HD uint32_t dm_piece(uint32_t R, uint32_t o)
{
    const uint32_t q = R / 258u, r = R % 258u;
    if (r == 0 || r >= 3) { if (o % 258u) return 0; return R - o < 258u ? R - o : 258u; }
    if (o == R - 3) return 3;                                          // r is 1 or 2 (so q >= 1): the last two pieces are 255 + r and 3
    if (o % 258u || o > R - 3) return 0;
    return o == 258u * (q - 1) ? 255u + r : 258u;
}

// ---------------------------------------------------------------------------------------------------------------- the tables of one member
struct DmCodes {
    uint32_t lfreq[DM_NLL], dfreq[DM_ND], clfreq[DM_NCL];
    uint32_t lA[DM_NLL], dA[DM_ND + 2], clA[DM_NCL + 1];              // counts in ascending order, then code lengths in that order
    uint16_t lsrt[DM_NLL], dsrt[DM_ND + 2], clsrt[DM_NCL + 1];        // the symbols with a count, ascending by (count, symbol)
    uint16_t lcode[DM_NLL], dcode[DM_ND + 2], clcode[DM_NCL + 1];     // canonical codes, bit-reversed (DEFLATE sends a code's first bit first)
    uint16_t blc[3][16];                                              // codes per length
    uint8_t llen[DM_NLL], dlen[DM_ND + 2], cllen[DM_NCL + 1];
    uint32_t nlen, ndist, ncode;                                      // HLIT + 257, HDIST + 1, HCLEN + 4
    uint32_t hdr_bits, total_bits;                                    // of the dynamic block: up to the first token; with the tokens and the end-of-block code
    uint32_t stored;                                                  // the block goes out stored
};
// rank of symbol s among the symbols with a count, by (count, symbol)
IM_HD uint32_t dm_rank(const uint32_t *freq, int n, int s)
{
    const uint32_t f = freq[s]; uint32_t r = 0;
    for (int q = 0; q < n; q++) { const uint32_t g = freq[q]; r += (g && (g < f || (g == f && q < s))) ? 1u : 0u; }
    return r;
}
// A[0 .. used): counts ascending, srt: their symbols -> len[] (zero on entry) for a code of at most `limit` bits.  One symbol: a single code of one bit.
IM_HD void dm_lengths_sorted(uint32_t *A, const uint16_t *srt, int used, int limit, uint8_t *len, uint16_t *blc)
{
    if (used == 0) return;
    if (used == 1) { len[srt[0]] = 1; return; }
    // minimum-redundancy code lengths in place (Moffat, Katajainen: In-place calculation of minimum-redundancy codes, 1995)
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < used - 1; next++) {
        if (leaf >= used || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= used || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[used - 2] = 0;
    for (next = used - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, usedn = 0, dpth = 0;
    root = used - 2; next = used - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { usedn++; root--; }
        while (avbl > usedn) { A[next--] = (uint32_t)dpth; avbl--; }
        avbl = 2 * usedn; dpth++; usedn = 0;
    }
    // the limit: every longer code is counted at the limit, then one code at a time leaves the limit and the deepest shorter code takes a sibling,
    // until the code space is exactly full again
    for (int l = 0; l <= 15; l++) blc[l] = 0;
    for (int i = 0; i < used; i++) blc[(int)A[i] > limit ? limit : (int)A[i]]++;
    uint32_t total = 0;
    for (int l = limit; l > 0; l--) total += (uint32_t)blc[l] << (limit - l);
    while (total != (1u << limit)) {
        blc[limit]--;
        for (int l = limit - 1; l > 0; l--) if (blc[l]) { blc[l]--; blc[l + 1] += 2; break; }
        total--;
    }
    int j = used;                                                      // the shortest codes to the largest counts
    for (int l = 1; l <= limit; l++) for (int k = blc[l]; k > 0; k--) len[srt[--j]] = (uint8_t)l;
}
// host: sort, then the lengths
IM_HD void dm_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, uint32_t *A, uint16_t *srt, uint16_t *blc)
{
    int used = 0;
    for (int s = 0; s < n; s++) { len[s] = 0; if (freq[s]) { const uint32_t r = dm_rank(freq, n, s); srt[r] = (uint16_t)s; A[r] = freq[s]; used++; } }
    dm_lengths_sorted(A, srt, used, limit, len, blc);
}
IM_HD uint32_t dm_rev(uint32_t code, int n) { uint32_t r = 0; for (int k = 0; k < n; k++) { r = (r << 1) | (code & 1u); code >>= 1; } return r; }
// canonical codes of the lengths (RFC 1951 3.2.2), reversed
IM_HD void dm_canon(const uint8_t *len, int n, uint16_t *code, uint16_t *blc)
{
    for (int l = 0; l <= 15; l++) blc[l] = 0;
    for (int s = 0; s < n; s++) blc[len[s]]++;
    uint32_t c = 0, prev = 0;
    for (int l = 1; l <= 15; l++) { c = (c + prev) << 1; prev = blc[l]; blc[l] = (uint16_t)c; }      // blc[l]: the next code of length l
    for (int s = 0; s < n; s++) { const int l = len[s]; code[s] = l ? (uint16_t)dm_rev(blc[l]++, l) : (uint16_t)0; }
}

// ---------------------------------------------------------------------------------------------------------------- bits, LSB first
struct DmBits { uint8_t *out; uint32_t pos; uint64_t acc; int cnt; };
IM_HD void dm_put(DmBits &b, uint64_t v, int n)                       // n <= 48
{
    b.acc |= v << b.cnt; b.cnt += n;
    while (b.cnt >= 8) { b.out[b.pos++] = (uint8_t)b.acc; b.acc >>= 8; b.cnt -= 8; }
}
IM_HD void dm_flush(DmBits &b) { if (b.cnt > 0) { b.out[b.pos++] = (uint8_t)b.acc; b.acc = 0; b.cnt = 0; } }

// ---------------------------------------------------------------------------------------------------------------- the block header
// The nlen + ndist code lengths as symbols of the code-length code, greedily: a run of zeros goes as 18 (11 .. 138) while 11 or more are left, then as 17
// (3 .. 10), then as single zeros; a run of another length goes as the length once, then 16 (3 .. 6) while 3 or more are left, then as single lengths.
// b == nullptr: the symbols are counted into clfreq; else they are written.
IM_HD uint32_t dm_seq(const DmCodes &w, uint32_t i) { return i < w.nlen ? w.llen[i] : w.dlen[i - w.nlen]; }
IM_HD void dm_cl(DmCodes &w, DmBits *b, int sym, uint32_t extra, int ebits)
{
    if (!b) { w.clfreq[sym]++; return; }
    dm_put(*b, w.clcode[sym], w.cllen[sym]);
    if (ebits) dm_put(*b, extra, ebits);
}
IM_HD void dm_rle(DmCodes &w, DmBits *b)
{
    const uint32_t n = w.nlen + w.ndist;
    for (uint32_t i = 0; i < n;) {
        const uint32_t v = dm_seq(w, i); uint32_t r = 1;
        while (i + r < n && dm_seq(w, i + r) == v) r++;
        uint32_t left = r;
        if (v == 0) {
            while (left >= 11) { const uint32_t t = left < 138 ? left : 138; dm_cl(w, b, 18, t - 11, 7); left -= t; }
            if (left >= 3) { dm_cl(w, b, 17, left - 3, 3); left = 0; }
        } else {
            dm_cl(w, b, (int)v, 0, 0); left--;
            while (left >= 3) { const uint32_t t = left < 6 ? left : 6; dm_cl(w, b, 16, t - 3, 2); left -= t; }
        }
        while (left) { dm_cl(w, b, (int)v, 0, 0); left--; }
        i += r;
    }
}
// After llen / dlen: HLIT / HDIST, the code-length code, all three sets of codes, the cost of the dynamic block, and whether n bytes go out stored instead
IM_HD void dm_finish_codes(DmCodes &w, uint32_t n)
{
    w.nlen = DM_NLL; while (w.nlen > 257 && w.llen[w.nlen - 1] == 0) w.nlen--;
    w.ndist = DM_ND; while (w.ndist > 1 && w.dlen[w.ndist - 1] == 0) w.ndist--;
    for (int s = 0; s < DM_NCL; s++) w.clfreq[s] = 0;
    dm_rle(w, nullptr);
    dm_lengths(w.clfreq, DM_NCL, 7, w.cllen, w.clA, w.clsrt, w.blc[2]);
    w.ncode = DM_NCL; while (w.ncode > 4 && w.cllen[im_clorder((int)w.ncode - 1)] == 0) w.ncode--;
    dm_canon(w.llen, DM_NLL, w.lcode, w.blc[0]);
    dm_canon(w.dlen, DM_ND, w.dcode, w.blc[1]);
    dm_canon(w.cllen, DM_NCL, w.clcode, w.blc[2]);
    uint32_t bits = 3 + 14 + 3 * w.ncode;
    for (int s = 0; s < DM_NCL; s++) bits += w.clfreq[s] * ((uint32_t)w.cllen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
    w.hdr_bits = bits;
    for (int s = 0; s < DM_NLL; s++) bits += w.lfreq[s] * ((uint32_t)w.llen[s] + (s > 256 ? (uint32_t)im_lext(s - 257) : 0u));
    for (int s = 0; s < DM_ND; s++) bits += w.dfreq[s] * ((uint32_t)w.dlen[s] + (uint32_t)im_dext(s));
    w.total_bits = bits;
    w.stored = ((bits + 7) >> 3) >= n + 5 ? 1u : 0u;
}
// BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code lengths in their order, the code lengths
IM_HD void dm_put_header(DmBits &b, DmCodes &w)
{
    dm_put(b, 1, 1); dm_put(b, 2, 2);
    dm_put(b, w.nlen - 257, 5); dm_put(b, w.ndist - 1, 5); dm_put(b, w.ncode - 4, 4);
    for (uint32_t k = 0; k < w.ncode; k++) dm_put(b, w.cllen[im_clorder((int)k)], 3);
    dm_rle(w, &b);
}
// the two halves of a match: code and extra bits of the length (at most 20 bits), of the distance (at most 28)
IM_HD uint32_t dm_len_bits(const DmCodes &w, uint32_t len, int *nbits)
{
    const int s = dm_lsym(len), n = w.llen[257 + s];
    *nbits = n + im_lext(s);
    return (uint32_t)w.lcode[257 + s] | ((len - im_lbase(s)) << n);
}
IM_HD uint32_t dm_dist_bits(const DmCodes &w, uint32_t dist, int *nbits)
{
    const int d = dm_dsym(dist), n = w.dlen[d];
    *nbits = n + im_dext(d);
    return (uint32_t)w.dcode[d] | ((dist - im_dbase(d)) << n);
}

// ---------------------------------------------------------------------------------------------------------------- CRC-32 in parts
// a * b mod P in the reflected representation of the gzip CRC (bit 31 is x^0)
IM_HD uint32_t dm_gfmul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1; }
    return p;
}
// x^(8 nbytes) mod P: crc(A B) = crc(A) * x^(8 |B|) + crc(B), and the CRC of no bytes is 0
IM_HD uint32_t dm_xpow8(uint32_t nbytes)
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    while (nbytes) { if (nbytes & 1u) r = dm_gfmul(r, sq); sq = dm_gfmul(sq, sq); nbytes >>= 1; }
    return r;
}
IM_HD uint32_t dm_crc_bytes(const uint8_t *p, uint32_t n, const uint32_t *crctab)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < n; k++) c = crctab[(c ^ p[k]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
// the CRC-32 of text[0 .. n) from the CRCs of its DM_CRC_CHUNK-byte chunks (the kernel folds the full chunks as a tree, this is the same product in a row)
IM_HD uint32_t dm_crc_chunked(const uint8_t *text, uint32_t n, const uint32_t *crctab)
{
    if (n == 0) return 0;
    const uint32_t last = (n - 1) / DM_CRC_CHUNK, X = dm_xpow8(DM_CRC_CHUNK);
    uint32_t acc = 0;
    for (uint32_t t = 0; t < last; t++) acc = dm_gfmul(acc, X) ^ dm_crc_bytes(text + t * DM_CRC_CHUNK, DM_CRC_CHUNK, crctab);
    const uint32_t lastlen = n - last * DM_CRC_CHUNK;
    return dm_gfmul(acc, dm_xpow8(lastlen)) ^ dm_crc_bytes(text + last * DM_CRC_CHUNK, lastlen, crctab);
}

// ---------------------------------------------------------------------------------------------------------------- the frame
// byte k < 18 of the header of a member of bsize + 1 bytes: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0 BSIZE
IM_HD uint8_t dm_header_byte(uint32_t k, uint32_t bsize)
{
    if (k < 8) return (uint8_t)(0x0000000004088b1full >> (8 * k));
    if (k < 16) return (uint8_t)(0x000243420006ff00ull >> (8 * (k - 8)));
    return (uint8_t)(bsize >> (8 * (k - 16)));
}
// byte k < 28 of the end-of-file marker: an empty member, its CDATA a fixed block that holds the end-of-block code alone (03 00)
IM_HD uint8_t dm_eof_byte(uint32_t k) { return k < 18 ? dm_header_byte(k, 27) : k == 18 ? (uint8_t)3 : (uint8_t)0; }
// byte k < 5 in front of the text of a stored block: BFINAL = 1, BTYPE = 0, LEN, ~LEN
IM_HD uint8_t dm_stored_byte(uint32_t k, uint32_t n) { return k == 0 ? (uint8_t)1 : k < 3 ? (uint8_t)(n >> (8 * (k - 1))) : (uint8_t)(~n >> (8 * (k - 3))); }
// bytes of BGZF that n bytes of text take at most: every member stored, and the marker
IM_HD uint64_t dm_bound(uint64_t n) { return (n + DM_TEXT - 1) / DM_TEXT * (uint64_t)DM_MEMBER_MAX + 28u; }

// ---------------------------------------------------------------------------------------------------------------- one member, in a row (host)
// tok: a literal is its byte; a match is 1 << 31 | length << 15 | distance - 1
struct DmHost { DmCodes w; uint16_t dist[DM_TEXT]; uint32_t tok[DM_TEXT]; uint32_t ntok; };
IM_HD uint32_t dm_tok_len(uint32_t t) { return (t >> 15) & 0xFFFFu; }
IM_HD uint32_t dm_tok_dist(uint32_t t) { return (t & 0x7FFFu) + 1u; }
IM_HD void dm_tokens(const uint8_t *text, uint32_t n, DmHost &H)
{
    uint32_t s0 = 0, s1 = DM_NONE, s2 = DM_NONE, s3 = DM_NONE, s4 = DM_NONE;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t D = dm_D(s0, s4);
        H.dist[j] = (uint16_t)((D && text[j] == text[j - D]) ? D : 0u);
        if (text[j] == '\n') { s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = j + 1; }
    }
    H.ntok = 0;
    for (uint32_t j = 0; j < n;) {
        const uint32_t d = H.dist[j]; uint32_t R = 1;
        if (d) while (j + R < n && H.dist[j + R] == d) R++;
        if (!d || R < DM_MINRUN) { for (uint32_t k = 0; k < R; k++) H.tok[H.ntok++] = text[j + k]; }
        else for (uint32_t o = 0; o < R;) { const uint32_t l = dm_piece(R, o); H.tok[H.ntok++] = 0x80000000u | (l << 15) | (d - 1); o += l; }
        j += R;
    }
}
// text[0 .. n), 1 <= n <= DM_TEXT -> the member at out (DM_MEMBER_MAX bytes suffice; fewer when the caller knows: nothing past the returned size is written
// by a member that goes out stored, a dynamic one is smaller than that).  -> its size
IM_HD uint32_t dm_member(const uint8_t *text, uint32_t n, uint8_t *out, DmHost &H, const uint32_t *crctab)
{
    DmCodes &w = H.w;
    dm_tokens(text, n, H);
    for (int s = 0; s < DM_NLL; s++) w.lfreq[s] = 0;
    for (int s = 0; s < DM_ND; s++) w.dfreq[s] = 0;
    w.lfreq[256] = 1;
    for (uint32_t i = 0; i < H.ntok; i++) {
        const uint32_t t = H.tok[i];
        if (t >> 31) { w.lfreq[257 + dm_lsym(dm_tok_len(t))]++; w.dfreq[dm_dsym(dm_tok_dist(t))]++; } else w.lfreq[t]++;
    }
    dm_lengths(w.lfreq, DM_NLL, 15, w.llen, w.lA, w.lsrt, w.blc[0]);
    dm_lengths(w.dfreq, DM_ND, 15, w.dlen, w.dA, w.dsrt, w.blc[1]);
    dm_finish_codes(w, n);
    uint32_t clen;
    if (w.stored) {
        clen = n + 5;
        for (uint32_t k = 0; k < 5; k++) out[18 + k] = dm_stored_byte(k, n);
        for (uint32_t k = 0; k < n; k++) out[23 + k] = text[k];
    } else {
        DmBits b; b.out = out + 18; b.pos = 0; b.acc = 0; b.cnt = 0;
        dm_put_header(b, w);
        for (uint32_t i = 0; i < H.ntok; i++) {
            const uint32_t t = H.tok[i];
            if (t >> 31) {
                int nb; uint32_t v = dm_len_bits(w, dm_tok_len(t), &nb); dm_put(b, v, nb);
                v = dm_dist_bits(w, dm_tok_dist(t), &nb); dm_put(b, v, nb);
            } else dm_put(b, w.lcode[t], w.llen[t]);
        }
        dm_put(b, w.lcode[256], w.llen[256]);
        dm_flush(b);
        clen = b.pos;
    }
    const uint32_t size = 18 + clen + 8, crc = dm_crc_chunked(text, n, crctab);
    for (uint32_t k = 0; k < 18; k++) out[k] = dm_header_byte(k, size - 1);
    for (uint32_t k = 0; k < 4; k++) { out[18 + clen + k] = (uint8_t)(crc >> (8 * k)); out[22 + clen + k] = (uint8_t)(n >> (8 * k)); }
    return size;
}
