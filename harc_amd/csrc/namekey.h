// namekey.h -- the name of a line (./harc -d -q -L NAMES; README: "-L and what it promises"), once for host and device: one rule for the id lines of an archive
// and for the lines of a list of names.  A line is taken without its newline, any bytes, '\r' a byte like any other:
//   1. a leading '@' is skipped;
//   2. the name runs up to, not including, the first space (0x20) or tab (0x09), or to the end of the line;
//   3. a name of at least 3 bytes that ends in "/1" or "/2" loses those two bytes, once ("a/1/2" gives "a/1").
// An empty name never matches.  The hash of a name is H = sum over its bytes of ck_term(o, name[o]) (check_block.h), o counted from the name's first byte: a sum of
// position-keyed terms, so lanes that each take eight bytes of a name add their parts in any order, and names of different lengths have different term sets.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "check_block.h"

#if defined(__HIPCC__)
#define NK_HD __host__ __device__ __forceinline__
#else
#define NK_HD static inline
#endif

#define NK_EMPTY 0xFFFFFFFFu                                      // the line word of a table slot that nobody has claimed
#define NK_MAX_LIST ((uint64_t)1 << 30)                           // bytes of a list of names: it is held whole in device memory

NK_HD bool nk_is_end(uint32_t b) { return b == 0x20u || b == 0x09u; }
// what rule 3 leaves of a name of `len` bytes whose last two bytes are b2, b1 (any values when len < 2)
NK_HD uint64_t nk_strip(uint64_t len, uint32_t b2, uint32_t b1) { return (len >= 3 && b2 == (uint32_t)'/' && (b1 == (uint32_t)'1' || b1 == (uint32_t)'2')) ? len - 2 : len; }
// the name of line[0 .. n): line[*off .. *off + *len)
NK_HD void nk_key(const uint8_t *line, uint64_t n, uint64_t *off, uint64_t *len)
{
    const uint64_t s = (n && line[0] == (uint8_t)'@') ? 1 : 0;
    uint64_t e = s;
    while (e < n && !nk_is_end(line[e])) e++;
    *off = s; *len = nk_strip(e - s, e - s >= 2 ? line[e - 2] : 0u, e - s >= 2 ? line[e - 1] : 0u);
}
NK_HD uint64_t nk_hash(const uint8_t *name, uint64_t len)
{
    uint64_t h = 0;
    for (uint64_t o = 0; o < len; o++) h += ck_term(o, name[o]);
    return h;
}
// HARC_AMD_SELECT_HASH_BITS (tests): the low `bits` bits of every H are kept, in the table and in the probe alike
NK_HD uint64_t nk_hash_mask(uint32_t bits) { return bits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << bits) - 1); }
// the slots of the table of `lines` list lines: the smallest power of two >= 2 * lines, at least 64
NK_HD uint64_t nk_table_slots(uint64_t lines) { uint64_t s = 64; while (s < 2 * lines) s <<= 1; return s; }

// ---- the host twins
// the lines of a text: (start, length without the newline) each; a last line without its newline counts as a line
static inline void nk_lines_host(const uint8_t *t, uint64_t n, std::vector<std::pair<uint64_t, uint64_t>> &out)
{
    out.clear();
    uint64_t i = 0;
    while (i < n) {
        const uint8_t *e = (const uint8_t *)memchr(t + i, '\n', (size_t)(n - i));
        const uint64_t end = e ? (uint64_t)(e - t) : n;
        out.emplace_back(i, end - i);
        i = end + 1;
    }
}
// The set of a list, as the device builds it: open addressing, linear probing, a slot owned by the FIRST list line that carries its name.
struct NkHostSet {
    const uint8_t *names = nullptr; uint64_t hmask = ~(uint64_t)0, mask = 63;
    std::vector<std::pair<uint64_t, uint64_t>> key;               // per list line: where its name is, its length
    std::vector<uint64_t> H;
    std::vector<uint32_t> slot_line; std::vector<uint64_t> slot_hash;
    std::vector<uint8_t> hit;                                     // per list line: it owns a slot and an id line carried its name
    uint64_t distinct = 0, skipped = 0;
    void build(const uint8_t *t, uint64_t n, uint32_t hash_bits)
    {
        names = t; hmask = nk_hash_mask(hash_bits);
        std::vector<std::pair<uint64_t, uint64_t>> lines;
        nk_lines_host(t, n, lines);
        const uint64_t slots = nk_table_slots(lines.size());
        mask = slots - 1;
        slot_line.assign((size_t)slots, NK_EMPTY); slot_hash.assign((size_t)slots, 0);
        key.resize(lines.size()); H.resize(lines.size()); hit.assign(lines.size(), 0);
        for (size_t l = 0; l < lines.size(); l++) {
            uint64_t off = 0, len = 0;
            nk_key(t + lines[l].first, lines[l].second, &off, &len);
            key[l] = std::make_pair(lines[l].first + off, len);
            H[l] = nk_hash(t + key[l].first, len) & hmask;
            if (!len) { skipped++; continue; }
            for (uint64_t s = H[l] & mask;; s = (s + 1) & mask) {
                const uint32_t o = slot_line[(size_t)s];
                if (o == NK_EMPTY) { slot_line[(size_t)s] = (uint32_t)l; slot_hash[(size_t)s] = H[l]; distinct++; break; }
                if (H[o] == H[l] && key[o].second == len && !memcmp(t + key[o].first, t + key[l].first, (size_t)len)) break;      // a duplicate
            }
        }
    }
    // the list line that owns the name, NK_EMPTY when the list does not hold it
    uint32_t find(const uint8_t *name, uint64_t len) const
    {
        if (!len) return NK_EMPTY;
        const uint64_t h = nk_hash(name, len) & hmask;
        for (uint64_t s = h & mask;; s = (s + 1) & mask) {
            const uint32_t o = slot_line[(size_t)s];
            if (o == NK_EMPTY) return NK_EMPTY;
            if (slot_hash[(size_t)s] == h && key[o].second == len && !memcmp(names + key[o].first, name, (size_t)len)) return o;
        }
    }
};
// flags[i] = id line i carries a listed name (one byte a line, room for every line of the id text); out = { id lines, distinct names, names found }
static inline void nk_select_flags_host(const uint8_t *names, uint64_t names_bytes, const uint8_t *ids, uint64_t id_bytes, uint32_t hash_bits, uint8_t *flags, uint64_t out[3], NkHostSet *set_out = nullptr)
{
    NkHostSet local, &S = set_out ? *set_out : local;
    S.build(names, names_bytes, hash_bits);
    std::vector<std::pair<uint64_t, uint64_t>> lines;
    nk_lines_host(ids, id_bytes, lines);
    uint64_t found = 0;
    for (size_t i = 0; i < lines.size(); i++) {
        uint64_t off = 0, len = 0;
        nk_key(ids + lines[i].first, lines[i].second, &off, &len);
        const uint32_t o = S.find(ids + lines[i].first + off, len);
        flags[i] = o != NK_EMPTY;
        if (o != NK_EMPTY && !S.hit[o]) { S.hit[o] = 1; found++; }
    }
    out[0] = lines.size(); out[1] = S.distinct; out[2] = found;
}
static inline uint64_t nk_count_lines_host(const uint8_t *t, uint64_t n)
{
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) k += t[i] == '\n';
    return k + ((n && t[n - 1] != '\n') ? 1 : 0);
}
// The selected lines of a text, compacted: stride > 0: line i is bytes [i * stride, (i + 1) * stride) (the text is n_lines * stride bytes); stride 0: lines of any
// length, each copied with its newline (a last line without one as it is).  out == nullptr: only the size.  Returns the bytes of the result
static inline uint64_t nk_gather_host(const uint8_t *t, uint64_t n, uint64_t stride, const uint8_t *flags, uint64_t n_lines, uint8_t *out)
{
    uint64_t w = 0;
    if (stride) {
        for (uint64_t i = 0; i < n_lines; i++) if (flags[i]) { if (out) memcpy(out + w, t + i * stride, (size_t)stride); w += stride; }
        return w;
    }
    uint64_t i = 0, line = 0;
    while (i < n && line < n_lines) {
        const uint8_t *e = (const uint8_t *)memchr(t + i, '\n', (size_t)(n - i));
        const uint64_t end = e ? (uint64_t)(e - t) + 1 : n;
        if (flags[line]) { if (out) memcpy(out + w, t + i, (size_t)(end - i)); w += end - i; }
        i = end; line++;
    }
    return w;
}
