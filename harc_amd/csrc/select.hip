// select.hip -- the records of an archive chosen by name on the GPU (./harc -d -q -L NAMES; README: "-L and what it promises").  The rule is namekey.h's.
//   k_nk_list_keys  a thread per list line: where its name is, its length, its hash
//   k_nk_claim      a thread per list line claims a slot of an open-addressing table with one 32-bit atomicCAS on the slot's line word, linear probing; a claimer
//                   that finds the slot taken compares its name with the owner's (hash and length from the per-line records, then the bytes): equal names
//                   leave the slot to the lower list line (atomicMin: the owner is the FIRST line that carries the name, whoever won the race), different ones
//                   probe on.  Nothing reads a slot's hash while claims are in flight:
//   k_nk_fill       a thread per slot, behind the claims: the owner's hash and length into the slot, the owners marked, the occupied slots counted
//   k_name_probe    the hot kernel, a streaming read of the id text through its line index in the manner of k_idm_rule: NK_G lanes a line, 8 bytes a lane and step
//                   (aligned 8-byte loads funnelled into place), the end of the name from a byte mask of spaces and tabs and a minimum over the group, the
//                   "/1" / "/2" strip from the two bytes in front of it, the hash summed over the lanes, the table walked with the group comparing bytes on an
//                   equal hash; one byte of flags a line, hit[owner] = 1 from whoever matches.  No atomics.
//   k_stride_gather lines of one length compacted, output-centric: a lane owns 16 bytes of the output
//   k_lines_len / k_lines_copy   lines of any length compacted (the pattern of k_q_copy of ingest.hip) behind a scan of their lengths
// The file call keeps the flags of the whole job resident, one byte a line, and walks every file through the context's pinned ring in pieces of whole lines.
#include "devutil.h"
#include "fileio.h"
#include "idmate.h"
#include "namekey.h"

#define NK_G 8
#define NK_NOPOS 0xFFFFFFFFu

struct alignas(16) NkSlot { unsigned long long hash; unsigned int line; unsigned int len; };
struct alignas(16) NkRec { uint32_t off, len; unsigned long long H; };       // per list line: its name's first byte in the list, its length, its hash

// the k (1 .. 8) bytes at p, the others zero; only aligned words that hold one of them are read
__device__ __forceinline__ uint64_t nk_fetch8(const uint8_t *p, uint32_t k)
{
    const uintptr_t u = (uintptr_t)p;
    const uint32_t sh = (uint32_t)(u & 7);
    const uint64_t *w = (const uint64_t *)(u - sh);
    uint64_t v = w[0] >> (8 * sh);
    if (sh + k > 8) v |= w[1] << (64 - 8 * sh);                   // (sh > 0 here)
    if (k < 8) v &= ((uint64_t)1 << (8 * k)) - 1;
    return v;
}
// 0x80 in every byte of x that is zero
__device__ __forceinline__ uint64_t nk_zero_bytes(uint64_t x)
{
    const uint64_t m = 0x7F7F7F7F7F7F7F7FULL;
    return ~(((x & m) + m) | x | m);
}

__global__ __launch_bounds__(256) void k_nk_list_keys(const uint8_t *names, const uint64_t *nls, uint32_t n, uint64_t hmask, NkRec *rec)
{
    const uint32_t l = harc_gid32();
    if (l >= n) return;
    const uint64_t s0 = nls[(int64_t)l - 1] + 1;
    uint64_t off = 0, len = 0;
    nk_key(names + s0, nls[l] - s0, &off, &len);
    NkRec r; r.off = (uint32_t)(s0 + off); r.len = (uint32_t)len; r.H = nk_hash(names + s0 + off, len) & hmask;
    rec[l] = r;
}
__device__ __forceinline__ bool nk_same_name(const uint8_t *names, const NkRec &a, const NkRec &b)
{
    if (a.H != b.H || a.len != b.len) return false;
    for (uint32_t j = 0; j < a.len; j++) if (names[a.off + j] != names[b.off + j]) return false;
    return true;
}
__global__ __launch_bounds__(256) void k_nk_claim(const uint8_t *names, const NkRec *rec, uint32_t n, NkSlot *slots, uint64_t mask)
{
    const uint32_t l = harc_gid32();
    if (l >= n) return;
    const NkRec me = rec[l];
    if (!me.len) return;
    for (uint64_t s = me.H & mask;; s = (s + 1) & mask) {
        const unsigned int old = atomicCAS(&slots[s].line, NK_EMPTY, l);
        if (old == NK_EMPTY) return;
        if (nk_same_name(names, me, rec[old])) { atomicMin(&slots[s].line, l); return; }      // (whoever owns the slot now carries the same name as `old`)
    }
}
__global__ __launch_bounds__(256) void k_nk_fill(NkSlot *slots, uint64_t nslots, const NkRec *rec, uint8_t *own, unsigned long long *count)
{
    const uint64_t s = harc_gid();
    bool used = false;
    if (s < nslots) {
        const unsigned int l = slots[s].line;
        if (l != NK_EMPTY) { used = true; slots[s].hash = rec[l].H; slots[s].len = rec[l].len; own[l] = 1; }
    }
    const unsigned long long b = __ballot(used);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

__device__ __forceinline__ uint32_t nk_group_min(uint32_t v)
{
#pragma unroll
    for (int o = 1; o < NK_G; o <<= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)v, o, 64); v = y < v ? y : v; }
    return v;
}

// line i of the id text (nls: its line index, nls[-1] = -1; a last line without its newline ends at the text's end) -> flags[i], hit[the list line that owns its name]
__global__ __launch_bounds__(256) void k_name_probe(const uint8_t *ids, const uint64_t *nls, uint64_t n, const uint8_t *names, const NkRec *rec, const NkSlot *slots,
                                                    uint64_t mask, uint64_t hmask, uint8_t *flags, uint8_t *hit)
{
    const uint64_t i = harc_gid() / NK_G;
    const uint32_t g = threadIdx.x & (NK_G - 1);
    const uint8_t *body = ids; uint32_t blen = 0;                 // the line behind its '@'
    if (i < n) {
        const uint64_t s0 = nls[(int64_t)i - 1] + 1, len = nls[i] - s0;
        const uint32_t at = (len && ids[s0] == (uint8_t)'@') ? 1u : 0u;
        body = ids + s0 + at; blen = (uint32_t)len - at;
    }
    // the end of the name: every lane walks its own chunks up to its first space or tab, the group takes the minimum (no shuffle inside the loop: the groups of
    // a wave have lines of different lengths).  The lane's first chunk stays in a register: a name of up to 64 bytes is read once
    uint32_t e = NK_NOPOS; uint64_t v0 = 0;
    for (uint32_t off = 8 * g; off < blen && e == NK_NOPOS; off += 8 * NK_G) {
        const uint32_t k = blen - off < 8 ? blen - off : 8;
        const uint64_t v = nk_fetch8(body + off, k);
        if (off == 8 * g) v0 = v;
        const uint64_t z = nk_zero_bytes(v ^ 0x2020202020202020ULL) | nk_zero_bytes(v ^ 0x0909090909090909ULL);      // (bytes behind k are zero: neither)
        if (z) e = off + ((uint32_t)__builtin_ctzll(z) >> 3);
    }
    e = nk_group_min(e);
    if (e > blen) e = blen;
    const uint32_t nlen = (uint32_t)nk_strip(e, e >= 2 ? body[e - 2] : 0u, e >= 2 ? body[e - 1] : 0u);
    // the hash: a sum of position-keyed terms, eight bytes a lane and step
    uint64_t h = 0;
    for (uint32_t off = 8 * g; off < nlen; off += 8 * NK_G) {
        const uint32_t k = nlen - off < 8 ? nlen - off : 8;
        const uint64_t v = off == 8 * g ? v0 : nk_fetch8(body + off, k);
        uint32_t nl = 0;
        ck_word(v, (1u << k) - 1u, off, &h, &nl);
    }
#pragma unroll
    for (int o = 1; o < NK_G; o <<= 1) h += (uint64_t)__shfl_xor((unsigned long long)h, o, 64);
    const uint64_t H = h & hmask;
    // the walk: slot H & mask, linear probing, the hash and the length first, then the group compares the bytes; an empty slot ends it.  The loop is uniform over
    // the wave (a group that is done idles), so that the shuffle inside it is executed by every lane
    bool done = !(i < n) || nlen == 0;
    uint32_t flag = 0; uint64_t s = H & mask;
    while (__any(!done)) {
        bool cmp = false; uint32_t owner = 0;
        if (!done) {
            const NkSlot sl = slots[s];
            if (sl.line == NK_EMPTY) done = true;
            else if (sl.hash != H || sl.len != nlen) s = (s + 1) & mask;
            else { cmp = true; owner = sl.line; }
        }
        uint32_t neq = 0;
        if (cmp) {
            const uint8_t *on = names + rec[owner].off;
            for (uint32_t off = 8 * g; off < nlen; off += 8 * NK_G) {
                const uint32_t k = nlen - off < 8 ? nlen - off : 8;
                const uint64_t a = off == 8 * g ? (k < 8 ? v0 & (((uint64_t)1 << (8 * k)) - 1) : v0) : nk_fetch8(body + off, k);
                neq |= a != nk_fetch8(on + off, k) ? 1u : 0u;
            }
        }
#pragma unroll
        for (int o = 1; o < NK_G; o <<= 1) neq |= (uint32_t)__shfl_xor((int)neq, o, 64);
        if (cmp) {
            if (!neq) { done = true; flag = 1; if (g == 0) hit[owner] = 1; }
            else s = (s + 1) & mask;
        }
    }
    if (i < n && g == 0) flags[i] = (uint8_t)flag;
}

// f[i] |= f[n + i], both ways: under the mate rule none a pair is selected when either of its id lines is
__global__ __launch_bounds__(256) void k_nk_or_halves(uint8_t *f, uint64_t n)
{
    const uint64_t i = harc_gid();
    if (i < n) { const uint8_t v = f[i] | f[n + i]; f[i] = v; f[n + i] = v; }
}
// *out += the bytes of p[0 .. n) that are not zero
__global__ __launch_bounds__(256) void k_nk_count(const uint8_t *p, uint64_t n, unsigned long long *out)
{
    const uint64_t i = harc_gid();
    const unsigned long long b = __ballot(i < n && p[i] != 0);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(out, (unsigned long long)__popcll(b));
}
__global__ __launch_bounds__(256) void k_nk_norm(const uint8_t *f, uint64_t n, uint8_t *f01)
{
    const uint64_t i = harc_gid();
    if (i < n) f01[i] = f[i] != 0;
}
// sel[pos[i]] = i for every flagged line
__global__ __launch_bounds__(256) void k_nk_sel(const uint8_t *f01, const uint64_t *pos, uint32_t n, uint32_t *sel)
{
    const uint32_t i = harc_gid32();
    if (i < n && f01[i]) sel[pos[i]] = i;
}

// Output byte o = byte (o mod S) of line sel[o / S] of src.  A lane owns the 16-byte chunk `chunk` of the hull of out[0 .. total): it collects its bytes in runs of
// up to 8 that stay inside one line, and writes them with one aligned 16-byte store; the first and the last chunk of a hull that is not aligned go byte by byte
__global__ __launch_bounds__(256) void k_stride_gather(const uint8_t *src, uint32_t S, const uint32_t *sel, uint8_t *out, uint64_t total)
{
    const uint64_t mis = (uint64_t)((uintptr_t)out & 15u), hull = mis + total, a = harc_gid() << 4;
    if (a >= hull) return;
    const uint32_t lo = a < mis ? (uint32_t)(mis - a) : 0u, hi = a + 16 > hull ? (uint32_t)(hull - a) : 16u;
    const uint64_t o = a + lo - mis;
    uint64_t j = o / S; uint32_t r = (uint32_t)(o - j * S);
    uint64_t w0 = 0, w1 = 0;
    for (uint32_t at = lo; at < hi;) {
        uint32_t k = 8 - (at & 7u);
        if (k > hi - at) k = hi - at;
        if (k > S - r) k = S - r;
        const uint64_t v = nk_fetch8(src + (uint64_t)sel[j] * S + r, k) << (8 * (at & 7u));
        if (at < 8) w0 |= v; else w1 |= v;
        at += k; r += k;
        if (r == S) { r = 0; j++; }
    }
    uint8_t *dst = out - mis + a;
    if (lo == 0 && hi == 16) *(uint4 *)dst = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    else for (uint32_t b = lo; b < hi; b++) dst[b] = (uint8_t)((b < 8 ? w0 >> (8 * b) : w1 >> (8 * (b - 8))) & 0xFFu);
}
// len[j] = the bytes of selected line j with its newline (a last line without one: as it is), len[m] = 0
__global__ __launch_bounds__(256) void k_lines_len(const uint64_t *nls, const uint32_t *sel, uint32_t m, uint64_t nbytes, uint32_t *len)
{
    const uint32_t j = harc_gid32();
    if (j > m) return;
    if (j == m) { len[j] = 0; return; }
    const int64_t li = (int64_t)sel[j];
    const uint64_t s = nls[li - 1] + 1, e = nls[li] + 1 < nbytes ? nls[li] + 1 : nbytes;
    len[j] = (uint32_t)(e - s);
}
// a wave per selected line
__global__ __launch_bounds__(256) void k_lines_copy(const uint8_t *txt, const uint64_t *nls, const uint32_t *sel, const uint32_t *len, const uint64_t *off, uint32_t m, uint8_t *out)
{
    const uint64_t j = harc_gid() >> 6;
    if (j >= m) return;
    const uint32_t lane = threadIdx.x & 63u, l = len[j];
    const uint8_t *s = txt + nls[(int64_t)sel[j] - 1] + 1;
    uint8_t *o = out + off[j];
    for (uint32_t b = lane; b < l; b += 64) o[b] = s[b];
}

// ------------------------------------------------------------------------------------------------ the set of a list, in pool memory of the caller's bracket
struct NkSet { const uint8_t *names = nullptr; NkRec *rec = nullptr; NkSlot *slots = nullptr; uint8_t *hit = nullptr, *own = nullptr; uint64_t lines = 0, mask = 0, hmask = 0, distinct = 0; };

static uint64_t nk_env_hmask()
{
    uint64_t b = env_u64("HARC_AMD_SELECT_HASH_BITS", 64);
    if (b > 64) b = 64;
    return nk_hash_mask((uint32_t)b);
}
static int nk_refuse_list(const char *who, uint64_t names_bytes)
{
    if (names_bytes <= NK_MAX_LIST) return HARC_AMD_OK;
    harc_set_error("%s: the list of names holds %llu bytes, more than the %llu that are held whole in device memory", who, (unsigned long long)names_bytes, (unsigned long long)NK_MAX_LIST);
    return HARC_AMD_EINVAL;
}
static int nk_build_set(harc_amd_ctx *c, const char *d_names, uint64_t names_bytes, NkSet *S)
{
    const uint64_t *nls = nullptr; bool open = false;
    S->names = (const uint8_t *)d_names; S->hmask = nk_env_hmask();
    RC_TRY(text_line_index(c, d_names, names_bytes, &nls, &S->lines, &open));
    const uint64_t slots = nk_table_slots(S->lines);
    S->mask = slots - 1;
    RC_TRY(dalloc(c, &S->rec, (size_t)S->lines + 1)); RC_TRY(dalloc(c, &S->slots, (size_t)slots));
    RC_TRY(dalloc(c, &S->hit, (size_t)S->lines + 1)); RC_TRY(dalloc(c, &S->own, (size_t)S->lines + 1));
    unsigned long long *d_cnt = nullptr; RC_TRY(dalloc(c, &d_cnt, 2));
    HIP_TRY(hipMemsetAsync(S->slots, 0xFF, (size_t)slots * sizeof(NkSlot), c->stream));      // (every line word NK_EMPTY)
    HIP_TRY(hipMemsetAsync(S->hit, 0, (size_t)S->lines + 1, c->stream)); HIP_TRY(hipMemsetAsync(S->own, 0, (size_t)S->lines + 1, c->stream));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 16, c->stream));
    if (S->lines) {
        const uint32_t n = (uint32_t)S->lines;
        hipLaunchKernelGGL(k_nk_list_keys, harc_grid256(n), dim3(256), 0, c->stream, S->names, nls, n, S->hmask, S->rec);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nk_claim, harc_grid256(n), dim3(256), 0, c->stream, S->names, (const NkRec *)S->rec, n, S->slots, S->mask);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nk_fill, harc_grid256(slots), dim3(256), 0, c->stream, S->slots, slots, (const NkRec *)S->rec, S->own, d_cnt);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    S->distinct = h;
    return HARC_AMD_OK;
}
static int nk_probe_launch(harc_amd_ctx *c, const NkSet &S, const char *d_ids, const uint64_t *nls, uint64_t n, uint8_t *d_flags)
{
    if (!n) return HARC_AMD_OK;
    hipLaunchKernelGGL(k_name_probe, harc_grid256(n * NK_G), dim3(256), 0, c->stream, (const uint8_t *)d_ids, nls, n, S.names, (const NkRec *)S.rec, (const NkSlot *)S.slots, S.mask, S.hmask, d_flags, S.hit);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}
// the bytes of p[0 .. n) that are not zero (the stream is waited for)
static int nk_count(harc_amd_ctx *c, const uint8_t *p, uint64_t n, uint64_t *out)
{
    *out = 0;
    if (!n) return HARC_AMD_OK;
    PoolScope scope(c);
    unsigned long long *d = nullptr; RC_TRY(dalloc(c, &d, 2));
    HIP_TRY(hipMemsetAsync(d, 0, 16, c->stream));
    hipLaunchKernelGGL(k_nk_count, harc_grid256(n), dim3(256), 0, c->stream, p, n, d);
    HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = h;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_name_key_host(const void *line, uint64_t n, uint64_t out[2])
{
    if (!out || (n && !line)) { harc_set_error("name_key_host: bad arguments"); return HARC_AMD_EINVAL; }
    nk_key((const uint8_t *)line, n, &out[0], &out[1]);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_select_flags_device(harc_amd_ctx *c, const void *d_names, uint64_t names_bytes, const void *d_ids, uint64_t id_bytes, uint8_t *d_flags,
                                            uint64_t *n_lines, uint64_t *n_names, uint64_t *n_found)
{
    if (!c || !n_lines || !n_names || !n_found || (names_bytes && !d_names) || (id_bytes && (!d_ids || !d_flags))) { harc_set_error("select_flags_device: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(nk_refuse_list("select_flags_device", names_bytes));
    if (id_bytes > 0xFFFFFFFFull) { harc_set_error("select_flags_device: %llu bytes of id text are more than the 2^32 - 1 of one call (a longer text goes in pieces: harc_amd_select_files)", (unsigned long long)id_bytes); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    NkSet S;
    RC_TRY(nk_build_set(c, (const char *)d_names, names_bytes, &S));
    const uint64_t *nls = nullptr; uint64_t lines = 0; bool open = false;
    RC_TRY(text_line_index(c, (const char *)d_ids, id_bytes, &nls, &lines, &open));
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    RC_TRY(nk_probe_launch(c, S, (const char *)d_ids, nls, lines, d_flags));
    RC_TRY(timer.end(c->stream));
    uint64_t found = 0;
    RC_TRY(nk_count(c, S.hit, S.lines, &found));
    if (trace) fprintf(stderr, "[select] device call: %llu id lines, %llu bytes of id text, %llu names in %llu slots, probe kernel %.3f ms (%.1f GB/s of id text)\n", (unsigned long long)lines,
                       (unsigned long long)id_bytes, (unsigned long long)S.distinct, (unsigned long long)(S.mask + 1), 1e3 * seconds, seconds > 0 ? 1e-9 * (double)id_bytes / seconds : 0.0);
    *n_lines = lines; *n_names = S.distinct; *n_found = found;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_select_flags_host(const void *names, uint64_t names_bytes, const void *ids, uint64_t id_bytes, uint8_t *flags, uint64_t *n_lines, uint64_t *n_names,
                                          uint64_t *n_found)
{
    if (!n_lines || !n_names || !n_found || (names_bytes && !names) || (id_bytes && (!ids || !flags))) { harc_set_error("select_flags_host: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(nk_refuse_list("select_flags_host", names_bytes));
    uint64_t hb = env_u64("HARC_AMD_SELECT_HASH_BITS", 64);
    uint64_t out[3] = { 0, 0, 0 };
    nk_select_flags_host((const uint8_t *)names, names_bytes, (const uint8_t *)ids, id_bytes, (uint32_t)(hb > 64 ? 64 : hb), flags, out);
    *n_lines = out[0]; *n_names = out[1]; *n_found = out[2];
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the gathers
static int nk_refuse_room(const char *who, uint64_t need, uint64_t capacity)
{
    if (need <= capacity) return HARC_AMD_OK;
    harc_set_error("%s: the selected lines take %llu bytes, the output has room for %llu", who, (unsigned long long)need, (unsigned long long)capacity);
    return HARC_AMD_EINVAL;
}
// The flagged lines (f01: 0 or 1 a line) of n_lines lines -> d_out, on the stream.  stride 0: nls is the text's line index.  The selected count is read back: one wait
static int nk_gather(harc_amd_ctx *c, const char *who, const char *d_text, uint64_t nbytes, uint64_t stride, const uint64_t *nls, const uint8_t *f01, uint64_t n_lines, char *d_out,
                     uint64_t capacity, uint64_t *out_bytes, uint64_t *out_lines = nullptr, double *seconds = nullptr)
{
    KernelTimer timer(seconds);
    *out_bytes = 0;
    if (out_lines) *out_lines = 0;
    if (!n_lines) return HARC_AMD_OK;
    PoolScope scope(c);
    uint64_t *pos = nullptr; RC_TRY(dalloc(c, &pos, (size_t)n_lines + 1));
    RC_TRY(prim_excl_scan_u8_to_u64(c, f01, pos, (size_t)n_lines));
    uint64_t before = 0; uint8_t last = 0;
    HIP_TRY(hipMemcpyAsync(&before, pos + (n_lines - 1), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&last, f01 + (n_lines - 1), 1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t m = before + last;
    if (out_lines) *out_lines = m;
    if (!m) return HARC_AMD_OK;
    uint32_t *sel = nullptr; RC_TRY(dalloc(c, &sel, (size_t)m + 1));
    hipLaunchKernelGGL(k_nk_sel, harc_grid256(n_lines), dim3(256), 0, c->stream, f01, (const uint64_t *)pos, (uint32_t)n_lines, sel);
    HIP_TRY(hipGetLastError());
    if (stride) {
        const uint64_t total = m * stride;
        RC_TRY(nk_refuse_room(who, total, capacity));
        RC_TRY(timer.begin(c->stream));
        hipLaunchKernelGGL(k_stride_gather, harc_grid256((total + 15 + 15) >> 4), dim3(256), 0, c->stream, (const uint8_t *)d_text, (uint32_t)stride, (const uint32_t *)sel, (uint8_t *)d_out, total);
        HIP_TRY(hipGetLastError());
        RC_TRY(timer.end(c->stream));
        *out_bytes = total;
    } else {
        uint32_t *len = nullptr; uint64_t *off = nullptr;
        RC_TRY(dalloc(c, &len, (size_t)m + 1)); RC_TRY(dalloc(c, &off, (size_t)m + 1));
        hipLaunchKernelGGL(k_lines_len, harc_grid256(m + 1), dim3(256), 0, c->stream, nls, (const uint32_t *)sel, (uint32_t)m, nbytes, len);
        HIP_TRY(hipGetLastError());
        RC_TRY(prim_excl_scan_u32_to_u64(c, len, off, (size_t)m + 1));
        uint64_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, off + m, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        RC_TRY(nk_refuse_room(who, total, capacity));
        RC_TRY(timer.begin(c->stream));
        hipLaunchKernelGGL(k_lines_copy, harc_grid256(m * 64), dim3(256), 0, c->stream, (const uint8_t *)d_text, nls, (const uint32_t *)sel, (const uint32_t *)len, (const uint64_t *)off, (uint32_t)m, (uint8_t *)d_out);
        HIP_TRY(hipGetLastError());
        RC_TRY(timer.end(c->stream));
        *out_bytes = total;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));                     // sel, len and off go with the scope
    return HARC_AMD_OK;
}

extern "C" int harc_amd_lines_gather_device(harc_amd_ctx *c, const void *d_text, uint64_t nbytes, uint64_t stride, const uint8_t *d_flags, uint64_t n_lines, void *d_out,
                                            uint64_t capacity, uint64_t *out_bytes)
{
    if (!c || !out_bytes || (nbytes && !d_text) || (n_lines && !d_flags) || (capacity && !d_out)) { harc_set_error("lines_gather_device: bad arguments"); return HARC_AMD_EINVAL; }
    *out_bytes = 0;
    if (nbytes > 0xFFFFFFFFull) { harc_set_error("lines_gather_device: %llu bytes are more than the 2^32 - 1 of one call", (unsigned long long)nbytes); return HARC_AMD_EINVAL; }
    if (stride && (stride > 0xFFFFFFFFull || n_lines > nbytes / stride || n_lines * stride != nbytes)) {
        harc_set_error("lines_gather_device: %llu lines of %llu bytes are not the %llu bytes of the text", (unsigned long long)n_lines, (unsigned long long)stride, (unsigned long long)nbytes);
        return HARC_AMD_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    const uint64_t *nls = nullptr;
    if (!stride) {
        uint64_t lines = 0; bool open = false;
        RC_TRY(text_line_index(c, (const char *)d_text, nbytes, &nls, &lines, &open));
        if (lines != n_lines) { harc_set_error("lines_gather_device: the text holds %llu lines, the flags are those of %llu", (unsigned long long)lines, (unsigned long long)n_lines); return HARC_AMD_EINVAL; }
    }
    if (!n_lines) return HARC_AMD_OK;
    uint8_t *f01 = nullptr; RC_TRY(dalloc(c, &f01, (size_t)n_lines));
    hipLaunchKernelGGL(k_nk_norm, harc_grid256(n_lines), dim3(256), 0, c->stream, d_flags, n_lines, f01);
    HIP_TRY(hipGetLastError());
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    RC_TRY(nk_gather(c, "lines_gather_device", (const char *)d_text, nbytes, stride, nls, f01, n_lines, (char *)d_out, capacity, out_bytes, nullptr, trace ? &seconds : nullptr));
    if (trace) fprintf(stderr, "[select] gather call: %llu lines of %llu bytes of text, %llu bytes gathered, %s kernel %.3f ms (%.1f GB/s of output)\n", (unsigned long long)n_lines, (unsigned long long)nbytes,
                       (unsigned long long)*out_bytes, stride ? "stride gather" : "line copy", 1e3 * seconds, seconds > 0 ? 1e-9 * (double)*out_bytes / seconds : 0.0);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_lines_gather_host(const void *text, uint64_t nbytes, uint64_t stride, const uint8_t *flags, uint64_t n_lines, void *out, uint64_t capacity, uint64_t *out_bytes)
{
    if (!out_bytes || (nbytes && !text) || (n_lines && !flags) || (capacity && !out)) { harc_set_error("lines_gather_host: bad arguments"); return HARC_AMD_EINVAL; }
    *out_bytes = 0;
    if (stride && (n_lines > nbytes / stride || n_lines * stride != nbytes)) {
        harc_set_error("lines_gather_host: %llu lines of %llu bytes are not the %llu bytes of the text", (unsigned long long)n_lines, (unsigned long long)stride, (unsigned long long)nbytes);
        return HARC_AMD_EINVAL;
    }
    if (!stride) {
        const uint64_t lines = nk_count_lines_host((const uint8_t *)text, nbytes);
        if (lines != n_lines) { harc_set_error("lines_gather_host: the text holds %llu lines, the flags are those of %llu", (unsigned long long)lines, (unsigned long long)n_lines); return HARC_AMD_EINVAL; }
    }
    const uint64_t need = nk_gather_host((const uint8_t *)text, nbytes, stride, flags, n_lines, nullptr);
    RC_TRY(nk_refuse_room("lines_gather_host", need, capacity));
    *out_bytes = nk_gather_host((const uint8_t *)text, nbytes, stride, flags, n_lines, (uint8_t *)out);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the files
// Phase B of harc_amd_select_files and of harc_amd_match_files (match.hip): every file of the job goes through the ring in pieces of whole lines, each piece is
// gathered by the resident flags and drained.  The id file (lines of any length; HARC_AMD_SELECT_PIECE bytes a piece) is walked by walk_lines of fileio.h, the
// files of lines of one length go HARC_AMD_SELECT_LINES lines a piece.  A job without an id file or without a quality file writes the others alone; a selection
// of nothing writes empty files.  An output file is removed unless the call reaches its end
int harc_gather_files(harc_amd_ctx *c, const GatherFiles &J)
{
    const bool have_ids = J.ids_path != nullptr, have_q = J.quality_path != nullptr;
    const uint64_t S = J.S, reads = J.reads, out_lines = J.out_lines;
    OutFileGuard guards[3] = { { have_ids ? J.out_ids_path : "" }, { J.out_dna_path }, { have_q ? J.out_quality_path : "" } };
    const bool have[3] = { have_ids, true, have_q };
    if (!have_ids) guards[0].ok = true;
    if (!have_q) guards[2].ok = true;
    if (!out_lines) {
        for (int k = 0; k < 3; k++) if (have[k]) RC_TRY(spit_file(guards[k].path, nullptr, 0));
        for (int k = 0; k < 3; k++) guards[k].ok = true;
        return HARC_AMD_OK;
    }
    DevBuf out{ c };
    if (have_ids) {
        // the ids: the size of the result is bounded by the file's; the drain cuts the file to what the pieces gave
        LineWalk w; w.piece = env_u64("HARC_AMD_SELECT_PIECE", (uint64_t)256 << 20); w.geom = J.feed; w.text_limit = 0xFFFFFFFFull; w.sync_turn = true;
        if (w.piece > ((uint64_t)1 << 30)) w.piece = (uint64_t)1 << 30;
        FileDrain drain(c);
        RC_TRY(drain.start(guards[0].path, (size_t)J.isz, &J.drain, true));
        uint64_t at = 0;
        RC_TRY(walk_lines(c, J.ids_path, J.isz, &w, [&](CarriedText &, LineTurn &t) -> int {
            if (t.line0 + t.whole > J.id_lines) return HARC_AMD_OK;  // (the file grew: refused below)
            RC_TRY(dev_reserve(&out, (size_t)t.cut));
            uint64_t got = 0;
            RC_TRY(nk_gather(c, J.who, t.text, t.cut, 0, t.nls, J.flags + t.line0, t.whole, out.p, t.cut, &got));
            if (got) RC_TRY(drain.put(out.p, (size_t)got, at));
            at += got;
            return HARC_AMD_OK;
        }));
        HIP_TRY(hipStreamSynchronize(c->stream));
        drain.set_final_size(at);
        RC_TRY(drain.finish());
        if (w.lines != J.id_lines && !J.ids_counted) { harc_set_error("%s: %s holds %llu lines, %llu are wanted: an id line per record", J.who, J.ids_path, (unsigned long long)w.lines, (unsigned long long)J.id_lines); return HARC_AMD_EINVAL; }
        if (w.lines != J.id_lines) { harc_set_error("%s: %s changed while it was read (%llu lines, then %llu)", J.who, J.ids_path, (unsigned long long)J.id_lines, (unsigned long long)w.lines); return HARC_AMD_EIO; }
        if (J.lap) J.lap->lap("ids gathered");
    }
    uint64_t PL = env_u64("HARC_AMD_SELECT_LINES", ((uint64_t)256 << 20) / S);
    if (PL * S > 0x7FFFFFFFull) PL = 0x7FFFFFFFull / S;
    const char *in_path[2] = { J.dna_path, J.quality_path };
    DevBuf txt{ c };
    RC_TRY(dev_reserve(&txt, (size_t)((reads < PL ? reads : PL) * S)));
    RC_TRY(dev_reserve(&out, (size_t)((reads < PL ? reads : PL) * S)));
    for (int k = 0; k < (have_q ? 2 : 1); k++) {
        FileDrain drain(c);
        RC_TRY(drain.start(guards[1 + k].path, (size_t)(out_lines * S), &J.drain));
        const Pieces pieces = line_pieces(reads, S, PL);
        FileFeeder feed(c, in_path[k]);
        RC_TRY(feed.start(pieces, J.feed));
        uint64_t at = 0;
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t bytes = pieces[p].second - pieces[p].first, line0 = pieces[p].first / S;
            RC_TRY(feed.upload_piece(p, txt.p, nullptr));
            uint64_t got = 0;
            RC_TRY(nk_gather(c, J.who, txt.p, bytes, S, nullptr, J.flags + line0, bytes / S, out.p, bytes, &got));
            if (at + got > out_lines * S) { harc_set_error("%s: %s gives more than the %llu selected lines", J.who, in_path[k], (unsigned long long)out_lines); return HARC_AMD_EINTERNAL; }
            if (got) RC_TRY(drain.put(out.p, (size_t)got, at));
            at += got;
            HIP_TRY(hipStreamSynchronize(c->stream));             // out and txt are written again by the next piece's upload and gather
        }
        RC_TRY(drain.finish());
        if (at != out_lines * S) { harc_set_error("%s: %s gave %llu bytes of selected lines, %llu were expected", J.who, in_path[k], (unsigned long long)at, (unsigned long long)(out_lines * S)); return HARC_AMD_EINTERNAL; }
        if (J.lap) J.lap->lap(k ? "quality gathered" : "reads gathered");
    }
    for (int k = 0; k < 3; k++) guards[k].ok = true;
    return HARC_AMD_OK;
}
// f[i] |= f[n + i], both ways, on the stream; the bytes of p[0 .. n) that are not zero (the stream is waited for): for match.hip
int harc_flags_or_halves(harc_amd_ctx *c, uint8_t *f, uint64_t n)
{
    if (!n) return HARC_AMD_OK;
    hipLaunchKernelGGL(k_nk_or_halves, harc_grid256(n), dim3(256), 0, c->stream, f, n);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}
int harc_flags_count(harc_amd_ctx *c, const uint8_t *p, uint64_t n, uint64_t *out) { return nk_count(c, p, n, out); }

// (the ids are walked in whole lines by walk_lines of fileio.h, twice: for the flags, then for the gather)
extern "C" int harc_amd_select_files(const harc_amd_params *params, const char *names_path, const char *ids_path, const char *dna_path, const char *quality_path,
                                     const char *out_ids_path, const char *out_dna_path, const char *out_quality_path, uint64_t pair_records, int32_t pair_rule,
                                     uint64_t stats[4], char *missing, uint64_t missing_cap)
{
    if (!params || !names_path || !ids_path || !dna_path || !quality_path || !out_ids_path || !out_dna_path || !out_quality_path || !stats) { harc_set_error("select_files: bad arguments"); return HARC_AMD_EINVAL; }
    if (pair_records && (pair_rule < IDM_NONE || pair_rule > IDM_SPACE)) { harc_set_error("select_files: %d is no mate rule (0 none, 1 same, 2 slash, 3 space)", (int)pair_rule); return HARC_AMD_EINVAL; }
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (missing && missing_cap) missing[0] = 0;
    uint64_t nsz = 0, isz = 0, dsz = 0, qsz = 0;
    if (!file_size(names_path, &nsz)) { harc_set_error("cannot open %s", names_path); return HARC_AMD_EIO; }
    if (!file_size(ids_path, &isz)) { harc_set_error("cannot open %s", ids_path); return HARC_AMD_EIO; }
    if (!file_size(dna_path, &dsz)) { harc_set_error("cannot open %s", dna_path); return HARC_AMD_EIO; }
    if (!file_size(quality_path, &qsz)) { harc_set_error("cannot open %s", quality_path); return HARC_AMD_EIO; }
    RC_TRY(nk_refuse_list("select_files", nsz));
    if (!nsz) { harc_set_error("select_files: the list of names %s is empty", names_path); return HARC_AMD_EINVAL; }
    uint32_t L = 0;
    RC_TRY(first_line_length(dna_path, "select_files", &L));
    const uint64_t S = (uint64_t)L + 1;
    if (dsz % S) { harc_set_error("select_files: the %llu bytes of %s are not lines of %u", (unsigned long long)dsz, dna_path, L); return HARC_AMD_EINVAL; }
    if (qsz != dsz) { harc_set_error("select_files: %s holds %llu bytes, %s %llu: a quality line per read is wanted", quality_path, (unsigned long long)qsz, dna_path, (unsigned long long)dsz); return HARC_AMD_EINVAL; }
    const uint64_t reads = dsz / S;
    if (reads > 0xFFFFFFFEull) { harc_set_error("select_files: %llu reads are more than one job holds", (unsigned long long)reads); return HARC_AMD_EINVAL; }
    const bool pair = pair_records != 0, once = pair && pair_rule != IDM_NONE;      // once: the id file holds file 1's ids alone
    if (pair && reads != 2 * pair_records) { harc_set_error("select_files: a pair of %llu records is wanted, %s holds %llu reads, not twice as many", (unsigned long long)pair_records, dna_path, (unsigned long long)reads); return HARC_AMD_EINVAL; }
    const uint64_t want_ids = once ? pair_records : reads, per_file = pair ? pair_records : reads;

    std::vector<uint8_t> list;
    if (!slurp_file(std::string(names_path), list, true)) return HARC_AMD_EIO;
    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    harc_amd_ctx *c = guard.c;
    const uint64_t big = isz > dsz ? isz : dsz;
    RingGeom g[2];                                                // a feeder and a drain are alive together
    RC_TRY(ring_split(c, 2, 8, "select", g, ring_slice_for(big, 8)));
    LapTimer lap{ "[select]" };
    PoolScope scope(c);
    DevBuf names{ c }, flags{ c };
    RC_TRY(dev_reserve(&names, list.size()));
    HIP_TRY(hipMemcpyAsync(names.p, list.data(), list.size(), hipMemcpyHostToDevice, c->stream));
    NkSet set;
    RC_TRY(nk_build_set(c, names.p, list.size(), &set));
    if (!set.distinct) { harc_set_error("select_files: no line of the list %s has a name (%llu lines)", names_path, (unsigned long long)set.lines); return HARC_AMD_EINVAL; }
    lap.lap("list and table");

    // ---- phase A: the flags of the whole job, one byte a line (a second half for the second file's records of a pair)
    RC_TRY(dev_reserve(&flags, (size_t)reads + 1));
    HIP_TRY(hipMemsetAsync(flags.p, 0, (size_t)reads + 1, c->stream));
    // a text at hand of more than 2^32 - 1 bytes is refused; the stream is waited for before a turn's line index goes
    LineWalk w; w.piece = env_u64("HARC_AMD_SELECT_PIECE", (uint64_t)256 << 20); w.geom = g[0]; w.text_limit = 0xFFFFFFFFull; w.sync_turn = true;
    if (w.piece > ((uint64_t)1 << 30)) w.piece = (uint64_t)1 << 30;
    double probe_s = 0;
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    {
        KernelTimer timer(trace ? &probe_s : nullptr);
        RC_TRY(walk_lines(c, ids_path, isz, &w, [&](CarriedText &, LineTurn &t) -> int {
            if (t.line0 + t.whole > want_ids) return HARC_AMD_OK;    // (more id lines than records: counted on, refused below)
            RC_TRY(timer.begin(c->stream));
            RC_TRY(nk_probe_launch(c, set, t.text, t.nls, t.whole, (uint8_t *)flags.p + t.line0));
            return timer.end(c->stream);
        }));
    }
    const uint64_t id_lines = w.lines;
    if (id_lines != want_ids) {
        if (pair) harc_set_error("select_files: %s holds %llu lines, a pair of %llu records under the rule %s has %llu", ids_path, (unsigned long long)id_lines, (unsigned long long)pair_records, idm_rule_name(pair_rule), (unsigned long long)want_ids);
        else harc_set_error("select_files: %s holds %llu lines, %s %llu reads: an id line per read is wanted", ids_path, (unsigned long long)id_lines, dna_path, (unsigned long long)reads);
        return HARC_AMD_EINVAL;
    }
    if (pair && !once) { hipLaunchKernelGGL(k_nk_or_halves, harc_grid256(per_file), dim3(256), 0, c->stream, (uint8_t *)flags.p, per_file); HIP_TRY(hipGetLastError()); }
    if (once) HIP_TRY(hipMemcpyAsync(flags.p + per_file, flags.p, (size_t)per_file, hipMemcpyDeviceToDevice, c->stream));
    uint64_t found = 0, selected = 0;
    RC_TRY(nk_count(c, set.hit, set.lines, &found));
    RC_TRY(nk_count(c, (const uint8_t *)flags.p, per_file, &selected));
    stats[0] = set.distinct; stats[1] = found; stats[2] = selected; stats[3] = per_file;
    if (trace) fprintf(stderr, "[select] %llu id lines probed in %.3f ms of kernels, %llu of %llu names found, %llu of %llu records selected\n", (unsigned long long)id_lines, 1e3 * probe_s,
                       (unsigned long long)found, (unsigned long long)set.distinct, (unsigned long long)selected, (unsigned long long)per_file);
    if (missing && missing_cap && found < set.distinct) {
        std::vector<uint8_t> own((size_t)set.lines), hit((size_t)set.lines); std::vector<NkRec> rec((size_t)set.lines);
        HIP_TRY(hipMemcpyAsync(own.data(), set.own, own.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hit.data(), set.hit, hit.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rec.data(), set.rec, rec.size() * sizeof(NkRec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        uint64_t w = 0; int shown = 0;
        for (size_t l = 0; l < own.size() && shown < 10; l++) {
            if (!own[l] || hit[l]) continue;
            if (w + rec[l].len + 2 > missing_cap) break;
            memcpy(missing + w, list.data() + rec[l].off, rec[l].len); w += rec[l].len; missing[w++] = '\n'; shown++;
        }
        missing[w] = 0;
    }
    lap.lap("phase A");

    // ---- phase B: every file in pieces of whole lines, each piece gathered and drained
    GatherFiles J;
    J.who = "select_files"; J.ids_path = ids_path; J.dna_path = dna_path; J.quality_path = quality_path;
    J.out_ids_path = out_ids_path; J.out_dna_path = out_dna_path; J.out_quality_path = out_quality_path;
    J.isz = isz; J.id_lines = id_lines; J.reads = reads; J.S = S; J.out_lines = pair ? 2 * selected : selected; J.flags = (const uint8_t *)flags.p;
    J.feed = g[0]; J.drain = g[1]; J.lap = &lap;
    return harc_gather_files(c, J);
}
