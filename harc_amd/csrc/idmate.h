// idmate.h -- the mate rule of paired-end ids (./harc -c R1 -2 R2 -p -q; README: "-2 and what it promises"), once for host and device.
// a = id line i of file 1, b = id line i of file 2, without their newlines, the '@' included, any bytes.  A pair satisfies at most one of
//   same    b == a
//   slash   |a| = |b| >= 2, a ends in "/1", b is a with its last byte '2'
//   space   |a| = |b|, a has a first space at s with s + 1 < |a|, a[s + 1] = '1', b is a with byte s + 1 set to '2'
// (slash and space both change exactly one byte; were it the same byte, the byte in front of it would be '/' and ' ' at once).  The rule of two files is the one
// that EVERY pair satisfies: the AND of the pairs' flag words; no pair at all gives same, no common rule gives none.  By construction apply(A, rule) == B.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define IDM_HD __host__ __device__ __forceinline__
#else
#define IDM_HD static inline
#endif

#define IDM_F_SAME 1u
#define IDM_F_SLASH 2u
#define IDM_F_SPACE 4u
#define IDM_F_ALL 7u
// the rules as numbers (include/harc_amd.h: HARC_AMD_IDMATE_*)
#define IDM_NONE 0
#define IDM_SAME 1
#define IDM_SLASH 2
#define IDM_SPACE 3
#define IDM_NOPOS 0xFFFFFFFFu

// What a pass over a pair of equally long lines has found -> the pair's flags.  ndiff: bytes that differ; p: where the first of them is; da, db: a[p], b[p];
// s: a's first space (IDM_NOPOS: none); a_before_last: a[len - 2] (any value when len < 2)
IDM_HD uint32_t idm_flags_of(uint32_t len, uint32_t ndiff, uint32_t p, uint32_t da, uint32_t db, uint32_t s, uint32_t a_before_last)
{
    if (ndiff == 0) return IDM_F_SAME;
    if (ndiff != 1 || da != (uint32_t)'1' || db != (uint32_t)'2') return 0;
    uint32_t f = 0;
    if (len >= 2 && p == len - 1 && a_before_last == (uint32_t)'/') f |= IDM_F_SLASH;
    if (s != IDM_NOPOS && s + 1 == p) f |= IDM_F_SPACE;
    return f;
}
IDM_HD int32_t idm_rule_of(uint32_t flags_and, uint64_t n_pairs)
{
    if (n_pairs == 0) return IDM_SAME;
    return (flags_and & IDM_F_SAME) ? IDM_SAME : (flags_and & IDM_F_SLASH) ? IDM_SLASH : (flags_and & IDM_F_SPACE) ? IDM_SPACE : IDM_NONE;
}
static inline const char *idm_rule_name(int32_t rule) { return rule == IDM_SAME ? "same" : rule == IDM_SLASH ? "slash" : rule == IDM_SPACE ? "space" : rule == IDM_NONE ? "none" : "?"; }
static inline int32_t idm_rule_parse(const char *s)
{
    for (int32_t r = IDM_NONE; r <= IDM_SPACE; r++) if (!strcmp(s, idm_rule_name(r))) return r;
    return -1;
}

// ---- the host twins, a line at a time
static inline uint32_t idm_pair_flags_host(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb)
{
    if (la != lb) return 0;
    uint32_t ndiff = 0, p = 0, s = IDM_NOPOS;
    for (uint64_t i = 0; i < la; i++) {
        if (a[i] != b[i] && ndiff++ == 0) p = (uint32_t)i;
        if (a[i] == ' ' && s == IDM_NOPOS) s = (uint32_t)i;
    }
    if (ndiff > 1) return 0;
    return idm_flags_of((uint32_t)la, ndiff, p, ndiff ? a[p] : 0, ndiff ? b[p] : 0, s, la >= 2 ? a[la - 2] : 0);
}
// the lines of a text: *lines = newlines, *open = a last line without one.  Line lengths above 2^32 - 2 do not occur in an id text the library handles
static inline void idm_count_lines_host(const uint8_t *t, uint64_t n, uint64_t *lines, int *open)
{
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) k += t[i] == '\n';
    *lines = k; *open = n && t[n - 1] != '\n';
}
// the AND over the pairs of two texts that hold the same number of closed lines
static inline uint32_t idm_rule_flags_host(const uint8_t *a, uint64_t an, const uint8_t *b, uint64_t bn)
{
    uint32_t f = IDM_F_ALL;
    uint64_t ia = 0, ib = 0;
    while (ia < an && ib < bn && f) {
        const uint8_t *ea = (const uint8_t *)memchr(a + ia, '\n', (size_t)(an - ia)), *eb = (const uint8_t *)memchr(b + ib, '\n', (size_t)(bn - ib));
        if (!ea || !eb) break;
        f &= idm_pair_flags_host(a + ia, (uint64_t)(ea - (a + ia)), b + ib, (uint64_t)(eb - (b + ib)));
        ia = (uint64_t)(ea - a) + 1; ib = (uint64_t)(eb - b) + 1;
    }
    return f;
}
// where the rule patches the line t[0 .. len): IDM_NOPOS when the line has no such byte
IDM_HD uint32_t idm_patch_pos(int32_t rule, uint32_t len, uint32_t first_space)
{
    if (rule == IDM_SLASH) return len ? len - 1 : IDM_NOPOS;
    if (rule == IDM_SPACE) return (first_space != IDM_NOPOS && first_space + 1 < len) ? first_space + 1 : IDM_NOPOS;
    return IDM_NOPOS;
}
// the closed lines of a text patched in place -> the lines whose byte was not '1' or that have none (they stay as they are)
static inline uint64_t idm_apply_host(uint8_t *t, uint64_t n, int32_t rule)
{
    if (rule != IDM_SLASH && rule != IDM_SPACE) return 0;
    uint64_t bad = 0, i = 0;
    while (i < n) {
        uint8_t *e = (uint8_t *)memchr(t + i, '\n', (size_t)(n - i));
        if (!e) break;
        const uint32_t len = (uint32_t)(e - (t + i));
        const uint8_t *sp = (const uint8_t *)memchr(t + i, ' ', len);
        const uint32_t p = idm_patch_pos(rule, len, sp ? (uint32_t)(sp - (t + i)) : IDM_NOPOS);
        if (p == IDM_NOPOS || t[i + p] != '1') bad++; else t[i + p] = '2';
        i += (uint64_t)len + 1;
    }
    return bad;
}
