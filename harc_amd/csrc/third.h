// third.h -- the rule of the third lines of a FASTQ file (./harc -c -q; README: "Third lines and what is promised"), once for host and device.
// a = the id line of a record, t = its third line, without their newlines, any bytes (a '\r' is a byte like any other).  A record satisfies
//   bare    |t| = 1 and t[0] = '+'
//   same    |t| = |a| >= 1, t[0] = '+' and t[1..] = a[1..] byte for byte (a[0] is not looked at)
// (a = "@", t = "+" satisfies both).  The rule of a job is the one that EVERY record satisfies: the AND of the records' flag words; no record at all gives bare,
// the bare bit left standing gives bare, otherwise the same bit gives same, otherwise the third lines are dropped (a mixed file is dropped).  A record takes part
// when its third line is there: a last record cut short behind line 1 or 2 does not, one cut short inside line 3 does, with what is left of that line.
// By construction '+' followed by a[1..] IS the third line under same: restoring needs no second check.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TH_HD __host__ __device__ __forceinline__
#else
#define TH_HD static inline
#endif

#define TH_F_BARE 1u
#define TH_F_SAME 2u
#define TH_F_ALL 3u
// the rules as numbers (include/harc_amd.h: HARC_AMD_THIRD_*)
#define TH_DROPPED 0
#define TH_BARE 1
#define TH_SAME 2
// first line of the archive member read.third; its second line is "third same" or "third dropped" (bare third lines leave no member)
#define TH_MAGIC "HARCT1"

// the flags of a record whose third line has length 1: its only byte and the length of the id line decide
TH_HD uint32_t th_flags_short(uint32_t t0, uint64_t la) { return t0 == (uint32_t)'+' ? (TH_F_BARE | (la == 1 ? TH_F_SAME : 0u)) : 0u; }
TH_HD int32_t th_rule_of(uint32_t flags_and, uint64_t n_records)
{
    if (n_records == 0) return TH_BARE;
    return (flags_and & TH_F_BARE) ? TH_BARE : (flags_and & TH_F_SAME) ? TH_SAME : TH_DROPPED;
}
static inline const char *th_rule_name(int32_t rule) { return rule == TH_BARE ? "bare" : rule == TH_SAME ? "same" : rule == TH_DROPPED ? "dropped" : "?"; }
static inline int32_t th_rule_parse(const char *s)
{
    for (int32_t r = TH_DROPPED; r <= TH_SAME; r++) if (!strcmp(s, th_rule_name(r))) return r;
    return -1;
}

// ---- the host twins, a record at a time
static inline uint32_t th_record_flags_host(const uint8_t *a, uint64_t la, const uint8_t *t, uint64_t lt)
{
    if (lt == 1) return th_flags_short(t[0], la);
    if (lt == 0 || lt != la || t[0] != (uint8_t)'+') return 0;
    return memcmp(a + 1, t + 1, (size_t)(la - 1)) ? 0u : TH_F_SAME;
}
// ... and a whole FASTQ text at a time: record r = lines 4 r .. 4 r + 3, a last line may lack its newline.  *n_records: the records that took part
static inline uint32_t th_text_flags_host(const uint8_t *txt, uint64_t n, uint64_t *n_records)
{
    uint32_t f = TH_F_ALL;
    uint64_t at = 0, recs = 0, k = 0, a0 = 0, la = 0;
    while (at < n) {
        const uint8_t *e = (const uint8_t *)memchr(txt + at, '\n', (size_t)(n - at));
        const uint64_t len = e ? (uint64_t)(e - (txt + at)) : n - at;
        if ((k & 3) == 0) { a0 = at; la = len; }
        else if ((k & 3) == 2) { f &= th_record_flags_host(txt + a0, la, txt + at, len); recs++; }
        at += len + 1; k++;
    }
    *n_records = recs;
    return f;
}
