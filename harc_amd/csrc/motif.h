// motif.h -- the rule of a match by sequence (./harc -d -M MOTIFS [-e K]; README: "-M and what it promises"), once for host and device.
// The list.  It is split at '\n'; a last line without its newline counts.  A line that is empty or begins with '>' is skipped.  Every other line is a motif: its bytes
//   are from ACGTNacgtn and are folded to upper case, any other byte ('\r' included) refuses the list, naming the line number and the byte.  A motif has 1 to 255
//   bases, and its cared bases, the ones that are not N, number more than K (otherwise every window would match: refused, naming the line).  Equal motifs count once.
//   At most 1024 distinct motifs, and a list of at most 2^20 bytes.
// The reverse complement.  rc(p) reverses p and exchanges A <-> T and C <-> G; N stays.
// A match.  Motif p of m bases matches read r of L bases when, for q = p or q = rc(p) and some offset 0 <= o <= L - m, #{ j : q[j] != 'N' and r[o + j] != q[j] } <= K.
//   A read byte that is N, or anything but A C G T, equals no motif base; under a motif's N nothing is compared; a motif longer than the reads matches nothing.
// The planes (match.hip).  A base has the 2-bit code (bit 1 of its byte, bit 2 of its byte): A 0,0  C 1,0  G 1,1  T 0,1.  Base j of a sequence is bit j & 31 of word
//   j >> 5 of the planes lo and hi; care (a motif) has the bit where the base is not N, bad (a read) where the byte is not one of A C G T.  Then the mismatches of a
//   window are the set bits of ((rlo ^ plo) | (rhi ^ phi) | rbad) & care.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MT_HD __host__ __device__ __forceinline__
#else
#define MT_HD static inline
#endif

#define MT_MAX_LEN 255u
#define MT_MAX_MOTIFS 1024u
#define MT_MAX_LIST ((uint64_t)1 << 20)
#define MT_MAX_K 8u
#define MT_WORDS 8                       // 32-bit words of a plane

MT_HD bool mt_is_base(uint32_t b) { return b == (uint32_t)'A' || b == (uint32_t)'C' || b == (uint32_t)'G' || b == (uint32_t)'T'; }
MT_HD uint32_t mt_lo(uint32_t b) { return (b >> 1) & 1u; }
MT_HD uint32_t mt_hi(uint32_t b) { return (b >> 2) & 1u; }
MT_HD uint8_t mt_complement(uint8_t b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b; }

// what goes to the device per motif and strand: its length, the motif of the list it stands for, its planes
// (word j of the three planes lies together, behind the head: a motif of up to 32 bases is 32 bytes in a row)
#define MT_LO 0
#define MT_HI 1
#define MT_CARE 2
struct alignas(16) MtEntry { uint32_t m, owner, pad[2]; uint32_t w[MT_WORDS][4]; };

// ---- the host's side: the list, the twin in byte comparisons, the table
#include <stdio.h>
#include <string>
#include <vector>

static inline std::string mt_rc(const std::string &p)
{
    std::string q(p.rbegin(), p.rend());
    for (char &ch : q) ch = (char)mt_complement((uint8_t)ch);
    return q;
}
// The distinct motifs of a list in list order, folded to upper case; false and the reason in `why` when the rule refuses the list
static inline bool mt_parse(const uint8_t *txt, uint64_t n, uint32_t K, std::vector<std::string> *motifs, std::string *why)
{
    char msg[256];
    motifs->clear();
    if (K > MT_MAX_K) { snprintf(msg, sizeof msg, "K = %u is more than the %u mismatches a match may have", K, MT_MAX_K); *why = msg; return false; }
    if (n > MT_MAX_LIST) { snprintf(msg, sizeof msg, "the list holds %llu bytes, more than the %llu of a list of motifs", (unsigned long long)n, (unsigned long long)MT_MAX_LIST); *why = msg; return false; }
    uint64_t at = 0, line = 0;
    while (at < n) {
        const uint8_t *e = (const uint8_t *)memchr(txt + at, '\n', (size_t)(n - at));
        const uint64_t len = e ? (uint64_t)(e - (txt + at)) : n - at;
        const uint8_t *l = txt + at;
        at += len + 1; line++;
        if (len == 0 || l[0] == (uint8_t)'>') continue;
        std::string p((size_t)len, 'N');
        uint32_t cared = 0;
        for (uint64_t j = 0; j < len; j++) {
            const uint8_t b = l[j] >= (uint8_t)'a' && l[j] <= (uint8_t)'z' ? (uint8_t)(l[j] - 32) : l[j];
            if (!mt_is_base(b) && b != (uint8_t)'N') { snprintf(msg, sizeof msg, "line %llu: byte 0x%02x is not one of ACGTNacgtn", (unsigned long long)line, (unsigned)l[j]); *why = msg; return false; }
            p[(size_t)j] = (char)b;
            cared += b != (uint8_t)'N';
        }
        if (len > MT_MAX_LEN) { snprintf(msg, sizeof msg, "line %llu: a motif of %llu bases is longer than %u", (unsigned long long)line, (unsigned long long)len, MT_MAX_LEN); *why = msg; return false; }
        if (cared <= K) {
            snprintf(msg, sizeof msg, "line %llu: the motif has %u bases that are not N, not more than the %u mismatches allowed: every window would match", (unsigned long long)line, cared, K);
            *why = msg; return false;
        }
        bool seen = false;
        for (const std::string &q : *motifs) if (q == p) { seen = true; break; }
        if (seen) continue;
        if (motifs->size() == MT_MAX_MOTIFS) { snprintf(msg, sizeof msg, "line %llu: more than %u distinct motifs", (unsigned long long)line, MT_MAX_MOTIFS); *why = msg; return false; }
        motifs->push_back(p);
    }
    if (motifs->empty()) { *why = "the list holds no motif"; return false; }
    return true;
}
// q against the L bytes at r, byte by byte
static inline bool mt_strand_matches(const std::string &q, const uint8_t *r, uint32_t L, uint32_t K)
{
    const uint32_t m = (uint32_t)q.size();
    if (m > L) return false;
    for (uint32_t o = 0; o + m <= L; o++) {
        uint32_t mis = 0;
        for (uint32_t j = 0; j < m && mis <= K; j++) if (q[j] != 'N' && r[o + j] != (uint8_t)q[j]) mis++;
        if (mis <= K) return true;
    }
    return false;
}
static inline bool mt_matches(const std::string &p, const uint8_t *r, uint32_t L, uint32_t K) { return mt_strand_matches(p, r, L, K) || mt_strand_matches(mt_rc(p), r, L, K); }
// flags[i] = some motif matches line i of the n lines of stride L + 1 at dna; hit[k] = motif k matches some line (hit is ORed into).  -> the lines selected
static inline uint64_t mt_flags_host(const std::vector<std::string> &motifs, uint32_t K, const uint8_t *dna, uint64_t n, uint32_t L, uint8_t *flags, uint8_t *hit)
{
    uint64_t selected = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint8_t f = 0;
        for (size_t k = 0; k < motifs.size(); k++) if (mt_matches(motifs[k], dna + i * ((uint64_t)L + 1), L, K)) { f = 1; hit[k] = 1; }
        flags[i] = f; selected += f;
    }
    return selected;
}
// the table of the device: every motif and its reverse complement (a palindrome twice: the flags do not change)
static inline void mt_entry_of(const std::string &q, uint32_t owner, MtEntry *e)
{
    memset(e, 0, sizeof *e);
    e->m = (uint32_t)q.size(); e->owner = owner;
    for (uint32_t j = 0; j < e->m; j++) {
        const uint32_t b = (uint8_t)q[j];
        if (b == (uint32_t)'N') continue;
        e->w[j >> 5][MT_LO] |= mt_lo(b) << (j & 31); e->w[j >> 5][MT_HI] |= mt_hi(b) << (j & 31); e->w[j >> 5][MT_CARE] |= 1u << (j & 31);
    }
}
static inline std::vector<MtEntry> mt_table(const std::vector<std::string> &motifs)
{
    std::vector<MtEntry> t(2 * motifs.size());
    for (size_t k = 0; k < motifs.size(); k++) { mt_entry_of(motifs[k], (uint32_t)k, &t[2 * k]); mt_entry_of(mt_rc(motifs[k]), (uint32_t)k, &t[2 * k + 1]); }
    return t;
}
