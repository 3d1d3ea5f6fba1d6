// gf_block.h -- the arithmetic of the recovery record (./harc -c -P, -R; README: "-P and what it promises", "The recovery record (X.hr)"), once for host and
// device: GF(2^8) over the polynomial 0x11D, the Cauchy coefficients, the geometry of blocks, spans and groups, the block digest, and -- host only -- the matrix
// inverse and the head of X.hr, built and read.  The reader validates every count against the size of the record before it allocates or reads anything by it.
#pragma once
#include <stdint.h>
#include <string.h>
#include "check_block.h"

#if defined(__HIPCC__)
#define GF_HD __host__ __device__ __forceinline__
#else
#define GF_HD static inline
#endif

#define GF_MAGIC "HARCR1\0\0"
#define GF_DEFAULT_B 65536u
#define GF_DEFAULT_S 8192u
#define GF_MAX_K 128u
#define GF_MAX_B (1u << 24)
#define GF_HEAD_FIXED 48u         // magic, B, S, K, PCT, files, 0, head_bytes, head_digest

// x * 2 on the four bytes of a word at once: the low seven bits of every byte move up, a byte whose high bit was set takes the polynomial's low byte 0x1D
GF_HD uint32_t gf_x2_word(uint32_t w)
{
    const uint32_t m = w & 0x80808080u;
    return ((w ^ m) << 1) ^ ((m - (m >> 7)) & 0x1D1D1D1Du);      // m - (m >> 7): 0x7F in every byte that had its high bit set
}
// the bytewise product, by doubling: no table
GF_HD uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    a &= 0xFFu;
    for (int k = 0; k < 8; k++) { if ((b >> k) & 1u) r ^= a; a = (a << 1) ^ ((a & 0x80u) ? 0x11Du : 0u); }
    return r & 0xFFu;
}
// c times each of the four bytes of w: the eight doublings of w, those named by the bits of c
GF_HD uint32_t gf_mul_word(uint32_t w, uint32_t c)
{
    uint32_t r = 0;
    for (int k = 0; k < 8; k++) { if ((c >> k) & 1u) r ^= w; w = gf_x2_word(w); }
    return r;
}
// a^254 = 1 / a for a != 0 (and 0 for 0)
GF_HD uint32_t gf_inv(uint32_t a)
{
    uint32_t r = 1, p = a & 0xFFu;                                // 254 = 0b11111110
    for (int k = 1; k < 8; k++) { p = gf_mul(p, p); r = gf_mul(r, p); }
    return r;
}
// the coefficient of member j in recovery block i of its group: i < 128 <= 128 + j, so i ^ (128 + j) is never 0 and the matrix is a Cauchy matrix
GF_HD uint32_t gf_cauchy(uint32_t i, uint32_t j) { return gf_inv(i ^ (128u + j)); }

// ---- geometry.  A file of n bytes: nb blocks of B; spans of at most S blocks; a span of s blocks: G groups, block t is member t / G of group t % G
struct GfGeom { uint32_t B, S, K, PCT; };
GF_HD uint64_t gf_blocks(uint64_t n, uint32_t B) { return n / B + (n % B ? 1 : 0); }
GF_HD uint64_t gf_spans(uint64_t nb, uint32_t S) { return nb / S + (nb % S ? 1 : 0); }
GF_HD uint32_t gf_span_blocks(uint64_t nb, uint32_t S, uint64_t sp) { const uint64_t left = nb - sp * S; return (uint32_t)(left < S ? left : S); }
GF_HD uint32_t gf_groups(uint32_t s, uint32_t K) { return (s + K - 1) / K; }
GF_HD uint32_t gf_group_members(uint32_t s, uint32_t G, uint32_t g) { return (s - g + G - 1) / G; }          // the t < s with t % G == g
GF_HD uint32_t gf_group_recovery(uint32_t k, uint32_t PCT) { const uint32_t m = (k * PCT + 99) / 100; return m < 1 ? 1 : m > 128 ? 128 : m; }
static inline bool gf_geom_ok(const GfGeom &g) { return g.B >= 16 && g.B <= GF_MAX_B && g.B % 16 == 0 && g.S >= 1 && g.S <= (1u << 24) && g.K >= 1 && g.K <= GF_MAX_K && g.PCT >= 1 && g.PCT <= 100; }
static inline uint32_t gf_span_recovery(uint32_t s, const GfGeom &g)
{
    const uint32_t G = gf_groups(s, g.K);
    uint32_t r = 0;
    for (uint32_t q = 0; q < G; q++) r += gf_group_recovery(gf_group_members(s, G, q), g.PCT);
    return r;
}
static inline uint64_t gf_file_recovery(uint64_t nb, const GfGeom &g)
{
    const uint64_t full = nb / g.S;
    uint64_t r = full ? full * gf_span_recovery(g.S, g) : 0;
    if (nb % g.S) r += gf_span_recovery((uint32_t)(nb % g.S), g);
    return r;
}
// the digest of a block: D of check_block.h with offsets counted from 0 inside the block, over its real bytes
static inline uint64_t gf_block_digest_host(const uint8_t *p, uint64_t len) { uint64_t acc[3] = { 0, 0, 0 }; ck_digest_host(p, len, 0, acc); return acc[2]; }

#include <string>
#include <vector>
// ---- the e x e matrix A over GF(2^8), row-major, inverted by elimination into inv; false: singular (a Cauchy matrix never is)
static inline bool gf_invert(const uint8_t *A, int e, uint8_t *inv)
{
    std::vector<uint8_t> M((size_t)e * e);
    memcpy(M.data(), A, (size_t)e * e);
    for (int r = 0; r < e; r++) for (int c = 0; c < e; c++) inv[r * e + c] = r == c;
    for (int col = 0; col < e; col++) {
        int piv = col;
        while (piv < e && !M[(size_t)piv * e + col]) piv++;
        if (piv == e) return false;
        if (piv != col) for (int c = 0; c < e; c++) { uint8_t t = M[(size_t)piv * e + c]; M[(size_t)piv * e + c] = M[(size_t)col * e + c]; M[(size_t)col * e + c] = t;
                                                       t = inv[piv * e + c]; inv[piv * e + c] = inv[col * e + c]; inv[col * e + c] = t; }
        const uint32_t d = gf_inv(M[(size_t)col * e + col]);
        for (int c = 0; c < e; c++) { M[(size_t)col * e + c] = (uint8_t)gf_mul(M[(size_t)col * e + c], d); inv[col * e + c] = (uint8_t)gf_mul(inv[col * e + c], d); }
        for (int r = 0; r < e; r++) {
            const uint32_t f = M[(size_t)r * e + col];
            if (r == col || !f) continue;
            for (int c = 0; c < e; c++) { M[(size_t)r * e + c] ^= (uint8_t)gf_mul(M[(size_t)col * e + c], f); inv[r * e + c] ^= (uint8_t)gf_mul(inv[col * e + c], f); }
        }
    }
    return true;
}
// The coefficients of one combine call that rebuilds the lost members of a group of k: lost[0 .. e) their member numbers, rec[0 .. e) the numbers i of the intact
// recovery blocks used.  The sources are the k - e intact members in ascending order, then the e recovery blocks: coef is e x k, row q for lost[q].
//   intact member j: sum over r of Ainv[q][r] * c(i_r, j);  recovery block i_r: Ainv[q][r],  A[r][q] = c(i_r, lost_q)
static inline bool gf_repair_coef(uint32_t k, const uint32_t *lost, const uint32_t *rec, int e, uint8_t *coef)
{
    std::vector<uint8_t> A((size_t)e * e), Ai((size_t)e * e);
    for (int r = 0; r < e; r++) for (int q = 0; q < e; q++) A[(size_t)r * e + q] = (uint8_t)gf_cauchy(rec[r], lost[q]);
    if (!gf_invert(A.data(), e, Ai.data())) return false;
    for (int q = 0; q < e; q++) {
        uint32_t s = 0; int nl = 0;
        for (uint32_t j = 0; j < k; j++) {
            if (nl < e && lost[nl] == j) { nl++; continue; }
            uint32_t v = 0;
            for (int r = 0; r < e; r++) v ^= gf_mul(Ai[(size_t)q * e + r], gf_cauchy(rec[r], j));
            coef[(size_t)q * k + s++] = (uint8_t)v;
        }
        for (int r = 0; r < e; r++) coef[(size_t)q * k + s++] = Ai[(size_t)q * e + r];
    }
    return true;
}

// ---- the head of X.hr (all integers little-endian):
//   "HARCR1\0\0", u32 B, S, K, PCT, files, 0, u64 head_bytes, u64 head_digest (D of the head with this field as zero);
//   per file u16 name_bytes, the name, u64 n, u64 D of the whole file, u64 nb, u64 recovery_blocks;
//   per file nb u64 data block digests, then recovery_blocks u64 recovery block digests.
// The record: the head, the recovery blocks (B bytes each; file, span, group, i), the head again, u64 head_bytes.
struct GfFile { std::string name; uint64_t n = 0, D = 0, nb = 0, rb = 0; std::vector<uint64_t> dd, rd; };
struct GfHead { GfGeom g = { 0, 0, 0, 0 }; std::vector<GfFile> files; uint64_t head_bytes = 0, recovery_blocks = 0; };
static inline void gf_put(std::vector<uint8_t> &o, uint64_t v, int bytes) { for (int k = 0; k < bytes; k++) o.push_back((uint8_t)(v >> (8 * k))); }
static inline uint64_t gf_get(const uint8_t *p, int bytes) { uint64_t v = 0; for (int k = 0; k < bytes; k++) v |= (uint64_t)p[k] << (8 * k); return v; }
static inline bool gf_name_ok(const std::string &s) { return !s.empty() && s.size() <= 65535 && s != "." && s != ".." && s.find('/') == std::string::npos && s.find('\0') == std::string::npos; }
static inline uint64_t gf_head_bytes(const std::vector<GfFile> &files)
{
    uint64_t hb = GF_HEAD_FIXED;
    for (const GfFile &f : files) hb += 2 + f.name.size() + 32 + 8 * (f.nb + f.rb);
    return hb;
}
static inline uint64_t gf_record_bytes(uint64_t hb, uint64_t recovery_blocks, uint32_t B) { return 2 * hb + recovery_blocks * B + 8; }
static inline std::vector<uint8_t> gf_head_build(const GfGeom &g, const std::vector<GfFile> &files)
{
    std::vector<uint8_t> o;
    const uint64_t hb = gf_head_bytes(files);
    o.reserve((size_t)hb);
    const char *magic = GF_MAGIC;
    o.insert(o.end(), magic, magic + 8);
    gf_put(o, g.B, 4); gf_put(o, g.S, 4); gf_put(o, g.K, 4); gf_put(o, g.PCT, 4); gf_put(o, files.size(), 4); gf_put(o, 0, 4);
    gf_put(o, hb, 8); gf_put(o, 0, 8);
    for (const GfFile &f : files) { gf_put(o, f.name.size(), 2); o.insert(o.end(), f.name.begin(), f.name.end()); gf_put(o, f.n, 8); gf_put(o, f.D, 8); gf_put(o, f.nb, 8); gf_put(o, f.rb, 8); }
    for (const GfFile &f : files) { for (uint64_t d : f.dd) gf_put(o, d, 8); for (uint64_t d : f.rd) gf_put(o, d, 8); }
    const uint64_t d = gf_block_digest_host(o.data(), o.size());
    for (int k = 0; k < 8; k++) o[40 + k] = (uint8_t)(d >> (8 * k));
    return o;
}
// One copy of the head, hb bytes at p, of a record of record_bytes bytes -> *h.  Nothing is allocated by a count that has not been held against hb first
static inline bool gf_head_parse(const uint8_t *p, uint64_t hb, uint64_t record_bytes, GfHead *h, std::string *why)
{
    if (hb < GF_HEAD_FIXED || memcmp(p, GF_MAGIC, 8)) { *why = "no magic HARCR1"; return false; }
    if (gf_get(p + 32, 8) != hb) { *why = "its length field does not name its length"; return false; }
    {
        uint64_t acc[3] = { 0, 0, 0 }; const uint8_t zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        ck_digest_host(p, 40, 0, acc); ck_digest_host(zero, 8, 40, acc); ck_digest_host(p + 48, hb - 48, 48, acc);
        if (acc[2] != gf_get(p + 40, 8)) { *why = "its digest does not hold"; return false; }
    }
    h->g = GfGeom{ (uint32_t)gf_get(p + 8, 4), (uint32_t)gf_get(p + 12, 4), (uint32_t)gf_get(p + 16, 4), (uint32_t)gf_get(p + 20, 4) };
    const uint64_t nf = gf_get(p + 24, 4);
    if (!gf_geom_ok(h->g) || gf_get(p + 28, 4)) { *why = "B, S, K or PCT out of range"; return false; }
    if (nf > (hb - GF_HEAD_FIXED) / 35) { *why = "more files than its bytes can name"; return false; }
    h->files.clear(); h->head_bytes = hb; h->recovery_blocks = 0;
    uint64_t at = GF_HEAD_FIXED, words = 0;
    for (uint64_t f = 0; f < nf; f++) {
        if (hb - at < 2) { *why = "the file entries leave the head"; return false; }
        const uint64_t nl = gf_get(p + at, 2); at += 2;
        if (hb - at < nl + 32) { *why = "the file entries leave the head"; return false; }
        GfFile F;
        F.name.assign((const char *)p + at, (size_t)nl); at += nl;
        F.n = gf_get(p + at, 8); F.D = gf_get(p + at + 8, 8); F.nb = gf_get(p + at + 16, 8); F.rb = gf_get(p + at + 24, 8); at += 32;
        if (!gf_name_ok(F.name)) { *why = "a file name that is empty, '.', '..' or holds a '/'"; return false; }
        for (const GfFile &o : h->files) if (o.name == F.name) { *why = "a file named twice"; return false; }
        if (F.nb != gf_blocks(F.n, h->g.B) || F.nb > hb / 8 || F.rb > hb / 8) { *why = "block counts that do not fit the file's length or the head"; return false; }
        if (F.rb != gf_file_recovery(F.nb, h->g)) { *why = "a recovery block count that does not follow from the file's blocks"; return false; }
        words += F.nb + F.rb; h->recovery_blocks += F.rb;
        if (words > hb / 8) { *why = "more digests than its bytes hold"; return false; }
        h->files.push_back(F);
    }
    if (hb - at != 8 * words) { *why = "digests that do not fill the head exactly"; return false; }
    if (h->recovery_blocks > record_bytes / h->g.B || gf_record_bytes(hb, h->recovery_blocks, h->g.B) != record_bytes) { *why = "counts that do not give the record's size"; return false; }
    for (GfFile &F : h->files) {
        F.dd.resize((size_t)F.nb); F.rd.resize((size_t)F.rb);
        for (uint64_t k = 0; k < F.nb; k++, at += 8) F.dd[(size_t)k] = gf_get(p + at, 8);
        for (uint64_t k = 0; k < F.rb; k++, at += 8) F.rd[(size_t)k] = gf_get(p + at, 8);
    }
    return true;
}
// The head of a record of `size` bytes that rd(offset, bytes, dst) reads: the first copy whose own digest holds and that parses.  *which: 1 or 2
template <class Rd> static inline bool gf_head_find(Rd rd, uint64_t size, GfHead *h, int *which, std::string *why)
{
    std::string w1 = "the record is shorter than a head", w2 = w1;
    uint8_t fix[GF_HEAD_FIXED];
    std::vector<uint8_t> buf;
    if (size >= 2 * (uint64_t)GF_HEAD_FIXED + 8) {
        if (rd(0, GF_HEAD_FIXED, fix)) {
            const uint64_t hb = gf_get(fix + 32, 8);
            if (memcmp(fix, GF_MAGIC, 8)) w1 = "no magic HARCR1";
            else if (hb < GF_HEAD_FIXED || hb > (size - 8) / 2) w1 = "a length that leaves the record";
            else { buf.resize((size_t)hb); if (!rd(0, hb, buf.data())) w1 = "cannot be read"; else if (gf_head_parse(buf.data(), hb, size, h, &w1)) { *which = 1; return true; } }
        } else w1 = "cannot be read";
        uint8_t tail[8];
        if (rd(size - 8, 8, tail)) {
            const uint64_t hb = gf_get(tail, 8);
            if (hb < GF_HEAD_FIXED || hb > (size - 8) / 2) w2 = "a length that leaves the record";
            else { buf.resize((size_t)hb); if (!rd(size - 8 - hb, hb, buf.data())) w2 = "cannot be read"; else if (gf_head_parse(buf.data(), hb, size, h, &w2)) { *which = 2; return true; } }
        } else w2 = "cannot be read";
    }
    *why = "neither copy of the head holds: the first copy: " + w1 + "; the second copy: " + w2;
    return false;
}
