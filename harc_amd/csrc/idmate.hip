// idmate.hip -- the mate rule of paired-end ids on the GPU (README: "-2 and what it promises").  The rule itself is idmate.h's; this file gives it its lanes.
//   k_idm_rule    a streaming compare of two id texts through their line indexes: IDM_G lanes per pair of lines, each lane takes 8 bytes of both lines per step
//                 (two aligned 8-byte loads funnelled into place, so that neither text needs an alignment), the group sums the differing bytes and finds the
//                 first of them and the first space, one lane turns that into the pair's flags, the wave ANDs its pairs and issues at most one atomicAnd.
//   k_idm_apply   the rule applied to the whole lines of a text in place (file 2's ids from file 1's): the same groups look for the byte to patch and count
//                 the lines that do not carry a '1' there.
// The file call walks the two id files in lockstep through the context's pinned ring; what a piece leaves behind its last paired line is carried on.
#include "devutil.h"
#include "fileio.h"
#include "idmate.h"

#define IDM_G 8

// the k (1 .. 8) bytes at p, the others zero; only aligned words that hold one of them are read
__device__ __forceinline__ uint64_t idm_fetch8(const uint8_t *p, uint32_t k)
{
    const uintptr_t u = (uintptr_t)p;
    const uint32_t sh = (uint32_t)(u & 7);
    const uint64_t *w = (const uint64_t *)(u - sh);
    uint64_t v = w[0] >> (8 * sh);
    if (sh + k > 8) v |= w[1] << (64 - 8 * sh);                   // (sh > 0 here)
    if (k < 8) v &= ((uint64_t)1 << (8 * k)) - 1;
    return v;
}
// bit 8 j + 7 for every byte j of x that is not zero
__device__ __forceinline__ uint64_t idm_nonzero_bytes(uint64_t x)
{
    const uint64_t m = 0x7F7F7F7F7F7F7F7FULL;
    return (((x & m) + m) | x) & ~m;
}
__device__ __forceinline__ uint32_t idm_group_min(uint32_t v)
{
#pragma unroll
    for (int o = 1; o < IDM_G; o <<= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)v, o, 64); v = y < v ? y : v; }
    return v;
}
// the first space of the line t[0 .. len) as the group sees it: every lane walks its own chunks, the group takes the minimum (no shuffle inside the loop:
// the groups of a wave have lines of different lengths)
__device__ __forceinline__ uint32_t idm_first_space(const uint8_t *t, uint32_t len, uint32_t g)
{
    uint32_t s = IDM_NOPOS;
    for (uint32_t off = 8 * g; off < len && s == IDM_NOPOS; off += 8 * IDM_G) {
        const uint32_t k = len - off < 8 ? len - off : 8;
        const uint64_t z = ~idm_nonzero_bytes(idm_fetch8(t + off, k) ^ 0x2020202020202020ULL) & 0x8080808080808080ULL;      // (bytes behind k are 0x20 ^ 0: no space)
        if (z) s = off + ((uint32_t)__builtin_ctzll(z) >> 3);
    }
    return idm_group_min(s);
}

// pair i = line i of both texts (nla / nlb: their line indexes, nl[-1] = -1).  *flags &= the flags of every pair
__global__ __launch_bounds__(256) void k_idm_rule(const uint8_t *a, const uint64_t *nla, const uint8_t *b, const uint64_t *nlb, uint64_t n, unsigned int *flags)
{
    const uint64_t i = harc_gid() / IDM_G;
    const uint32_t g = threadIdx.x & (IDM_G - 1);
    const uint8_t *pa = a, *pb = b;
    uint32_t len = 0; bool live = false, same_len = true;
    if (i < n) {
        const uint64_t sa = nla[(int64_t)i - 1] + 1, la = nla[i] - sa, sb = nlb[(int64_t)i - 1] + 1, lb = nlb[i] - sb;
        live = true; same_len = la == lb;
        if (same_len) { pa = a + sa; pb = b + sb; len = (uint32_t)la; }
    }
    uint32_t ndiff = 0, p = IDM_NOPOS, info = 0, s = IDM_NOPOS;
    for (uint32_t off = 8 * g; off < len; off += 8 * IDM_G) {
        const uint32_t k = len - off < 8 ? len - off : 8;
        const uint64_t va = idm_fetch8(pa + off, k), vb = idm_fetch8(pb + off, k);
        const uint64_t y = idm_nonzero_bytes(va ^ vb);
        if (y) {
            if (ndiff == 0) {
                const uint32_t j = (uint32_t)__builtin_ctzll(y) >> 3;
                p = off + j; info = ((uint32_t)(va >> (8 * j)) & 0xFFu) << 8 | ((uint32_t)(vb >> (8 * j)) & 0xFFu);
            }
            ndiff += (uint32_t)__popcll(y);
        }
        if (s == IDM_NOPOS) {
            const uint64_t z = ~idm_nonzero_bytes(va ^ 0x2020202020202020ULL) & 0x8080808080808080ULL;
            if (z) s = off + ((uint32_t)__builtin_ctzll(z) >> 3);
        }
    }
    // the group's sums and minima; with one differing byte in all, only its lane holds an info word
#pragma unroll
    for (int o = 1; o < IDM_G; o <<= 1) { ndiff += (uint32_t)__shfl_xor((int)ndiff, o, 64); info |= (uint32_t)__shfl_xor((int)info, o, 64); }
    p = idm_group_min(p); s = idm_group_min(s);
    uint32_t f = IDM_F_ALL;
    if (live) f = same_len ? idm_flags_of(len, ndiff, p, info >> 8, info & 0xFFu, s, len >= 2 ? pa[len - 2] : 0u) : 0u;
#pragma unroll
    for (int o = IDM_G; o < 64; o <<= 1) f &= (uint32_t)__shfl_xor((int)f, o, 64);
    // at most one atomic per wave, and none once the word holds no bit that this wave would clear: the waves of a file that follows a rule all carry the same flags,
    // and two million atomics on one address would be the kernel's whole time (a stale read only costs an atomic that changes nothing)
    if ((threadIdx.x & 63u) == 0 && (*(volatile unsigned int *)flags & ~f) != 0) atomicAnd(flags, f);
}

// lines [0, n) of t patched in place by `rule` (IDM_SLASH or IDM_SPACE); *bad += the lines that have no byte to patch or another one than '1' there
__global__ __launch_bounds__(256) void k_idm_apply(uint8_t *t, const uint64_t *nls, uint64_t n, int rule, unsigned long long *bad)
{
    const uint64_t i = harc_gid() / IDM_G;
    const uint32_t g = threadIdx.x & (IDM_G - 1);
    uint8_t *line = t; uint32_t len = 0;
    if (i < n) { const uint64_t s0 = nls[(int64_t)i - 1] + 1; line = t + s0; len = (uint32_t)(nls[i] - s0); }
    uint32_t s = IDM_NOPOS;
    if (rule == IDM_SPACE) s = idm_first_space(line, len, g);     // (every lane of the wave gets here)
    if (i < n && g == 0) {
        const uint32_t p = idm_patch_pos(rule, len, s);
        if (p == IDM_NOPOS || line[p] != (uint8_t)'1') atomicAdd(bad, 1ull); else line[p] = (uint8_t)'2';
    }
}

// ------------------------------------------------------------------------------------------------ launches, for this file and fastq_out.hip
static int idm_rule_launch(harc_amd_ctx *c, const char *d_a, const uint64_t *nla, const char *d_b, const uint64_t *nlb, uint64_t m, unsigned int *d_flags)
{
    if (!m) return HARC_AMD_OK;
    hipLaunchKernelGGL(k_idm_rule, harc_grid256(m * IDM_G), dim3(256), 0, c->stream, (const uint8_t *)d_a, nla, (const uint8_t *)d_b, nlb, m, d_flags);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}
int harc_idmate_apply_lines(harc_amd_ctx *c, char *d_ids, const uint64_t *nls, uint64_t m, int32_t rule, unsigned long long *d_bad)
{
    if (!m || (rule != IDM_SLASH && rule != IDM_SPACE)) return HARC_AMD_OK;
    hipLaunchKernelGGL(k_idm_apply, harc_grid256(m * IDM_G), dim3(256), 0, c->stream, (uint8_t *)d_ids, nls, m, (int)rule, d_bad);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}

static int idm_check_rule(const char *who, int32_t rule)
{
    if (rule >= IDM_NONE && rule <= IDM_SPACE) return HARC_AMD_OK;
    harc_set_error("%s: %d is no mate rule (0 none, 1 same, 2 slash, 3 space)", who, (int)rule);
    return HARC_AMD_EINVAL;
}
static int idm_refuse_counts(const char *who, uint64_t la, bool oa, uint64_t lb, bool ob)
{
    if (oa || ob) { harc_set_error("%s: the last line of the %s text has no newline (the texts hold %llu and %llu closed lines)", who, oa ? "first" : "second", (unsigned long long)la, (unsigned long long)lb); return HARC_AMD_EINVAL; }
    if (la != lb) { harc_set_error("%s: the first text holds %llu lines, the second %llu: mates are paired by their place", who, (unsigned long long)la, (unsigned long long)lb); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idmate_rule_device(harc_amd_ctx *c, const char *d_a, uint64_t a_bytes, const char *d_b, uint64_t b_bytes, uint64_t *n_pairs, uint32_t *flags_and)
{
    if (!c || !n_pairs || !flags_and || (a_bytes && !d_a) || (b_bytes && !d_b)) { harc_set_error("idmate_rule_device: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    const uint64_t *nla = nullptr, *nlb = nullptr; uint64_t la = 0, lb = 0; bool oa = false, ob = false;
    RC_TRY(text_line_index(c, d_a, a_bytes, &nla, &la, &oa)); RC_TRY(text_line_index(c, d_b, b_bytes, &nlb, &lb, &ob));
    RC_TRY(idm_refuse_counts("idmate_rule_device", la - (oa ? 1 : 0), oa, lb - (ob ? 1 : 0), ob));
    unsigned int *d_flags = nullptr; RC_TRY(dalloc(c, &d_flags, 4));
    HIP_TRY(hipMemsetAsync(d_flags, 0xFF, 16, c->stream));
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    RC_TRY(idm_rule_launch(c, d_a, nla, d_b, nlb, la, d_flags));
    RC_TRY(timer.end(c->stream));
    unsigned int f = 0;
    HIP_TRY(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (trace) fprintf(stderr, "[idmate] device call: %llu pairs, %llu bytes of both texts, rule kernel %.3f ms (%.1f GB/s)\n", (unsigned long long)la, (unsigned long long)(a_bytes + b_bytes),
                       1e3 * seconds, seconds > 0 ? 1e-9 * (double)(a_bytes + b_bytes) / seconds : 0.0);
    *n_pairs = la; *flags_and = f & IDM_F_ALL;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idmate_apply_device(harc_amd_ctx *c, char *d_ids, uint64_t id_bytes, int32_t rule, uint64_t *bad)
{
    if (!c || !bad || (id_bytes && !d_ids)) { harc_set_error("idmate_apply_device: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(idm_check_rule("idmate_apply_device", rule));
    *bad = 0;
    if (!id_bytes || rule == IDM_NONE || rule == IDM_SAME) return HARC_AMD_OK;
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    const uint64_t *nls = nullptr; uint64_t lines = 0; bool open = false;
    RC_TRY(text_line_index(c, d_ids, id_bytes, &nls, &lines, &open));
    unsigned long long *d_bad = nullptr; RC_TRY(dalloc(c, &d_bad, 2));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 16, c->stream));
    RC_TRY(harc_idmate_apply_lines(c, d_ids, nls, lines - (open ? 1 : 0), rule, d_bad));      // whole lines only
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *bad = h;
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the host twins
extern "C" int harc_amd_idmate_rule_host(const char *a, uint64_t a_bytes, const char *b, uint64_t b_bytes, uint64_t *n_pairs, uint32_t *flags_and)
{
    if (!n_pairs || !flags_and || (a_bytes && !a) || (b_bytes && !b)) { harc_set_error("idmate_rule_host: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t la = 0, lb = 0; int oa = 0, ob = 0;
    idm_count_lines_host((const uint8_t *)a, a_bytes, &la, &oa); idm_count_lines_host((const uint8_t *)b, b_bytes, &lb, &ob);
    RC_TRY(idm_refuse_counts("idmate_rule_host", la, oa != 0, lb, ob != 0));
    *n_pairs = la; *flags_and = idm_rule_flags_host((const uint8_t *)a, a_bytes, (const uint8_t *)b, b_bytes);
    return HARC_AMD_OK;
}
extern "C" int harc_amd_idmate_apply_host(char *ids, uint64_t id_bytes, int32_t rule, uint64_t *bad)
{
    if (!bad || (id_bytes && !ids)) { harc_set_error("idmate_apply_host: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(idm_check_rule("idmate_apply_host", rule));
    *bad = idm_apply_host((uint8_t *)ids, id_bytes, rule);
    return HARC_AMD_OK;
}
extern "C" int32_t harc_amd_idmate_rule_of(uint32_t flags_and, uint64_t n_pairs) { return idm_rule_of(flags_and, n_pairs); }
extern "C" const char *harc_amd_idmate_rule_name(int32_t rule) { return idm_rule_name(rule); }
extern "C" int32_t harc_amd_idmate_rule_parse(const char *name) { return name ? idm_rule_parse(name) : -1; }

// ------------------------------------------------------------------------------------------------ the files
// one of the two id files on its way through the GPU: its pieces, its feeder, its text with what the last turn left.  The steps of a turn (index, cut, carry) are
// CarriedText's (fileio.h); the lockstep of the two files is this file's
struct IdmSide {
    const char *path; uint64_t fsz = 0;
    Pieces pieces; size_t next = 0;
    FileFeeder feed; CarriedText txt;
    uint64_t total = 0, carry_lines = 0, lines_total = 0;         // bytes of this turn's text; whole lines carried into it; whole lines seen in all
    LineTurn t;                                                   // its line index and its whole lines: those that have their newline
    IdmSide(harc_amd_ctx *c, const char *p) : path(p), feed(c, p), txt(c) {}
    bool done() const { return next == pieces.size(); }
};

extern "C" int harc_amd_idmate_rule_files(const harc_amd_params *params, const char *path_a, const char *path_b, int32_t *rule, uint64_t *n_pairs)
{
    if (!params || !path_a || !path_b || !rule || !n_pairs) { harc_set_error("idmate_rule_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t asz = 0, bsz = 0;
    if (!file_size(path_a, &asz)) { harc_set_error("cannot open %s", path_a); return HARC_AMD_EIO; }
    if (!file_size(path_b, &bsz)) { harc_set_error("cannot open %s", path_b); return HARC_AMD_EIO; }
    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    harc_amd_ctx *c = guard.c;
    // two feeders alive at the same time: half of the ring each; files of a few MB do not pin a ring of 1 GiB
    RingGeom g[2];
    RC_TRY(ring_split(c, 2, 8, "id mates", g, ring_slice_for(asz > bsz ? asz : bsz, 8)));
    const uint64_t piece = env_u64("HARC_AMD_IDMATE_PIECE", (uint64_t)256 << 20);
    IdmSide A(c, path_a), B(c, path_b); A.fsz = asz; B.fsz = bsz;
    IdmSide *S[2] = { &A, &B };
    for (int k = 0; k < 2; k++) {
        S[k]->pieces = byte_pieces(0, S[k]->fsz, piece);
        if (!S[k]->pieces.empty()) RC_TRY(S[k]->feed.start(S[k]->pieces, g[k]));
    }
    PoolScope scope(c);
    unsigned int *d_flags = nullptr; RC_TRY(dalloc(c, &d_flags, 4));
    HIP_TRY(hipMemsetAsync(d_flags, 0xFF, 16, c->stream));
    double t_read = 0; uint64_t pairs = 0; int turns = 0;
    for (;;) {
        // a side takes its next piece when it holds no whole line any more or less than a piece of text: what it carries stays bounded by two pieces,
        // however differently the lines of the two files fall into the pieces
        bool took = false;
        for (int k = 0; k < 2; k++) {
            IdmSide &s = *S[k];
            s.total = s.txt.carry;
            if (s.done() || (s.carry_lines != 0 && s.txt.carry >= piece)) continue;
            const uint64_t len = s.pieces[s.next].second - s.pieces[s.next].first;
            RC_TRY(s.txt.take(s.feed, s.next, len, &t_read));
            s.total += len; s.next++; took = true;
        }
        if (!took) break;
        PoolScope turn_scope(c);
        for (int k = 0; k < 2; k++) {
            IdmSide &s = *S[k];
            RC_TRY(s.txt.index(s.total, false, &s.t));
            s.lines_total += s.t.whole - s.carry_lines;
        }
        const uint64_t m = A.t.whole < B.t.whole ? A.t.whole : B.t.whole;
        RC_TRY(idm_rule_launch(c, A.t.text, A.t.nls, B.t.text, B.t.nls, m, d_flags));
        pairs += m; turns++;
        for (int k = 0; k < 2; k++) {
            IdmSide &s = *S[k], &o = *S[k ^ 1];
            // lines whose partner can no longer come (the other file has ended and all its lines are paired) are counted and dropped
            const uint64_t use = (o.done() && o.t.whole == m) ? s.t.whole : m;
            uint64_t cut = 0;
            RC_TRY(s.txt.line_end(s.t.nls, use, &cut));
            RC_TRY(s.txt.carry_behind(cut, s.total));
            s.carry_lines = s.t.whole - use;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));                 // the line indexes go with the turn's scope
    }
    if (A.txt.carry || B.txt.carry) {
        harc_set_error("idmate_rule_files: the last line of %s has no newline (%llu and %llu closed lines)", A.txt.carry ? path_a : path_b, (unsigned long long)A.lines_total, (unsigned long long)B.lines_total);
        return HARC_AMD_EINVAL;
    }
    if (A.lines_total != B.lines_total) {
        harc_set_error("idmate_rule_files: %s holds %llu lines, %s %llu: mates are paired by their place", path_a, (unsigned long long)A.lines_total, path_b, (unsigned long long)B.lines_total);
        return HARC_AMD_EINVAL;
    }
    unsigned int f = 0;
    HIP_TRY(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (getenv("HARC_AMD_TRACE")) fprintf(stderr, "[idmate] %llu pairs in %d turns, %.3f s waiting for the readers\n", (unsigned long long)pairs, turns, t_read);
    *n_pairs = pairs; *rule = idm_rule_of(f & IDM_F_ALL, pairs);
    return HARC_AMD_OK;
}
