// match.hip -- the records of an archive chosen by the sequence of their reads on the GPU (./harc -d -M MOTIFS [-e K]; README: "-M and what it promises").  The rule
// is motif.h's.  The list is parsed on the host; the device gets a table of entries, every motif and its reverse complement: the length, the motif of the list it
// stands for, and the three bit planes lo, hi, care of up to 256 bits.
//   k_motif_match   the hot kernel over the reads as they lie in output.dna, lines of stride L + 1: MT_G lanes a read.
//                   Reads to planes: lane g turns bases [32 g, 32 g + 32) of its line into one 32-bit word of the planes lo, hi and bad (not ACGT) -- up to three
//                   aligned 16-byte loads funnelled into place, a load only where the chunk holds a byte of the line, so nothing outside the 16-byte hull of the text
//                   is read -- and the group exchanges the words with cross-lane moves: every lane then holds the read's planes, NW = ceil(L / 32) words each.
//                   Offsets: lane g takes the offsets o = g (mod MT_G): it shifts its planes once by g and then by the constant MT_G per step.
//                   Motif loop: per offset the lane walks the table; the step, the entry and the branch on the entry's words are the same for every lane of the
//                   wave, so the entry's planes come through scalar loads.  x = ((rlo ^ plo) | (rhi ^ phi) | rbad) & care, the popcounts over the motif's words are
//                   summed and compared with K; a window that ends behind the read does not count.
//                   Results: the group ORs its verdicts, one byte of flags a line; hit[owner] = 1 is a plain store from whoever matches.  No atomics, no early
//                   way out: flags and hits are a function of the two texts and K alone.
// The file call keeps the flags of the whole job resident, one byte a line, walks output.dna through the context's pinned ring in pieces of whole lines, and hands
// the flags to the gather that -L uses (select.hip: harc_gather_files).
#include "devutil.h"
#include "fileio.h"
#include "idmate.h"
#include "motif.h"

#define MT_G 8

// 0x80 in every byte of x that is zero
__device__ __forceinline__ uint32_t mt_zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
// bit k of byte j of w -> bit j of the result
__device__ __forceinline__ uint32_t mt_gather4(uint32_t w, int k) { return ((((w >> k) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; }
// the low word of { hi, lo } >> s, 0 <= s <= 31
__device__ __forceinline__ uint32_t mt_funnel(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_alignbit(hi, lo, s); }

// The nb (0 .. 32) bytes at p as one word of each plane; bits nb and above: lo, hi 0, bad 1.  Only aligned 16-byte chunks that hold one of the bytes are read
__device__ __forceinline__ void mt_pack32(const uint8_t *p, uint32_t nb, uint32_t *lo, uint32_t *hi, uint32_t *bad)
{
    *lo = 0; *hi = 0; *bad = 0xFFFFFFFFu;
    if (!nb) return;
    const uint32_t sh = (uint32_t)((uintptr_t)p & 15u);
    const uint4 *a = (const uint4 *)(p - sh);
    const uint4 z = make_uint4(0, 0, 0, 0);
    const uint4 q0 = a[0], q1 = sh + nb > 16 ? a[1] : z, q2 = sh + nb > 32 ? a[2] : z;
    uint32_t v[12] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };
    // the funnel: whole words by two selects with constant indices (the array stays in registers), then the bytes inside a word
    if (sh & 8u) {
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = k + 2 < 12 ? v[k + 2] : 0u;
    }
    if (sh & 4u) {
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = k + 1 < 12 ? v[k + 1] : 0u;
    }
    const uint32_t bs = (sh & 3u) * 8u;
    uint32_t l = 0, h = 0, b = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t w = mt_funnel(v[k + 1], v[k], bs);
        const uint32_t ok = mt_zero_bytes(w ^ 0x41414141u) | mt_zero_bytes(w ^ 0x43434343u) | mt_zero_bytes(w ^ 0x47474747u) | mt_zero_bytes(w ^ 0x54545454u);
        l |= mt_gather4(w, 1) << (4 * k); h |= mt_gather4(w, 2) << (4 * k); b |= mt_gather4(~ok, 7) << (4 * k);
    }
    const uint32_t in = nb >= 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
    *lo = l & in; *hi = h & in; *bad = b | ~in;
}

// the mismatches of the entry's first KW words against the planes
template <int KW, int NW> __device__ __forceinline__ uint32_t mt_score(const uint32_t (&rlo)[NW], const uint32_t (&rhi)[NW], const uint32_t (&rbad)[NW], const MtEntry &E)
{
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < KW; j++) cnt += (uint32_t)__popc(((rlo[j] ^ E.w[j][MT_LO]) | (rhi[j] ^ E.w[j][MT_HI]) | rbad[j]) & E.w[j][MT_CARE]);
    return cnt;
}

// line i of the n lines of stride L + 1 at text -> flags[i], hit[the motif that matches it]; NW = ceil(L / 32)
template <int NW> __global__ __launch_bounds__(256) void k_motif_match(const uint8_t *__restrict__ text, uint64_t n, uint32_t L, const MtEntry *__restrict__ tab, uint32_t ne, uint32_t K,
                                                                       uint8_t *__restrict__ flags, uint8_t *__restrict__ hit)
{
    const uint64_t i = harc_gid() / MT_G;
    const uint32_t g = threadIdx.x & (MT_G - 1);
    const bool live = i < n;
    // ---- reads to planes
    const uint32_t nb = live && L > 32u * g ? (L - 32u * g < 32u ? L - 32u * g : 32u) : 0u;
    uint32_t fl, fh, fb;
    mt_pack32(text + (live ? i * ((uint64_t)L + 1) + 32u * g : 0u), nb, &fl, &fh, &fb);
    uint32_t rlo[NW], rhi[NW], rbad[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) { rlo[j] = (uint32_t)__shfl((int)fl, j, MT_G); rhi[j] = (uint32_t)__shfl((int)fh, j, MT_G); rbad[j] = (uint32_t)__shfl((int)fb, j, MT_G); }
    // ---- the lane's residue
#pragma unroll
    for (int j = 0; j < NW; j++) {
        rlo[j] = mt_funnel(j + 1 < NW ? rlo[j + 1] : 0u, rlo[j], g); rhi[j] = mt_funnel(j + 1 < NW ? rhi[j + 1] : 0u, rhi[j], g);
        rbad[j] = mt_funnel(j + 1 < NW ? rbad[j + 1] : 0u, rbad[j], g);
    }
    // ---- offsets o = g + MT_G t, the table walked at each
    uint32_t flag = 0;
    for (uint32_t t = 0; t < L; t += MT_G) {                      // (t, e: the same in every lane)
        const uint32_t o = g + t;
        for (uint32_t e = 0; e < ne; e++) {
            const MtEntry &E = tab[e];
            const uint32_t m = E.m, kw = (m + 31u) >> 5;
            uint32_t cnt = mt_score<1, NW>(rlo, rhi, rbad, E);      // the first word with the entry's head, in one trip: motifs of up to 32 bases wait once
            if (kw > 1) {
                switch (kw) {
                case 2: if constexpr (NW >= 2) cnt = mt_score<2, NW>(rlo, rhi, rbad, E); break;
                case 3: if constexpr (NW >= 3) cnt = mt_score<3, NW>(rlo, rhi, rbad, E); break;
                case 4: if constexpr (NW >= 4) cnt = mt_score<4, NW>(rlo, rhi, rbad, E); break;
                case 5: if constexpr (NW >= 5) cnt = mt_score<5, NW>(rlo, rhi, rbad, E); break;
                case 6: if constexpr (NW >= 6) cnt = mt_score<6, NW>(rlo, rhi, rbad, E); break;
                case 7: if constexpr (NW >= 7) cnt = mt_score<7, NW>(rlo, rhi, rbad, E); break;
                default: if constexpr (NW >= 8) cnt = mt_score<8, NW>(rlo, rhi, rbad, E); break;
                }
            }
            if (live && o + m <= L && cnt <= K) { flag = 1; hit[E.owner] = 1; }      // (a motif of more words than the read has: o + m > L)
        }
#pragma unroll
        for (int j = 0; j < NW; j++) {
            rlo[j] = mt_funnel(j + 1 < NW ? rlo[j + 1] : 0u, rlo[j], MT_G); rhi[j] = mt_funnel(j + 1 < NW ? rhi[j + 1] : 0u, rhi[j], MT_G);
            rbad[j] = mt_funnel(j + 1 < NW ? rbad[j + 1] : 0u, rbad[j], MT_G);
        }
    }
#pragma unroll
    for (int s = 1; s < MT_G; s <<= 1) flag |= (uint32_t)__shfl_xor((int)flag, s, 64);
    if (live && g == 0) flags[i] = (uint8_t)flag;
}

// ------------------------------------------------------------------------------------------------ the list and its table
struct MtSet { std::vector<std::string> motifs; MtEntry *tab = nullptr; uint8_t *hit = nullptr; uint32_t K = 0; };

static int mt_parse_list(const char *who, const void *list, uint64_t list_bytes, uint32_t K, std::vector<std::string> *motifs)
{
    std::string why;
    if (mt_parse((const uint8_t *)list, list_bytes, K, motifs, &why)) return HARC_AMD_OK;
    harc_set_error("%s: %s", who, why.c_str());
    return HARC_AMD_EINVAL;
}
// the table and the hits of a parsed list in pool memory of the caller's bracket (the stream is waited for: the host table goes)
static int mt_load_set(harc_amd_ctx *c, MtSet *S)
{
    const std::vector<MtEntry> t = mt_table(S->motifs);
    RC_TRY(dalloc(c, &S->tab, t.size())); RC_TRY(dalloc(c, &S->hit, S->motifs.size()));
    HIP_TRY(hipMemcpyAsync(S->tab, t.data(), t.size() * sizeof(MtEntry), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(S->hit, 0, S->motifs.size(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HARC_AMD_OK;
}
static int mt_launch(harc_amd_ctx *c, const MtSet &S, const char *d_text, uint64_t n, uint32_t L, uint8_t *d_flags)
{
    if (!n) return HARC_AMD_OK;
    const dim3 grid = harc_grid256(n * MT_G);
    const uint32_t ne = (uint32_t)(2 * S.motifs.size());
#define MT_LAUNCH(NW) hipLaunchKernelGGL(k_motif_match<NW>, grid, dim3(256), 0, c->stream, (const uint8_t *)d_text, n, L, (const MtEntry *)S.tab, ne, S.K, d_flags, S.hit)
    switch ((L + 31u) >> 5) {
    case 1: MT_LAUNCH(1); break;
    case 2: MT_LAUNCH(2); break;
    case 3: MT_LAUNCH(3); break;
    case 4: MT_LAUNCH(4); break;
    case 5: MT_LAUNCH(5); break;
    case 6: MT_LAUNCH(6); break;
    case 7: MT_LAUNCH(7); break;
    default: MT_LAUNCH(8); break;
    }
#undef MT_LAUNCH
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}
// the hits of the set -> hit (host, may be null) and their count
static int mt_hits(harc_amd_ctx *c, const MtSet &S, std::vector<uint8_t> *h, uint64_t *found)
{
    h->assign(S.motifs.size(), 0);
    HIP_TRY(hipMemcpyAsync(h->data(), S.hit, h->size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *found = 0;
    for (uint8_t b : *h) *found += b != 0;
    return HARC_AMD_OK;
}
static int mt_refuse_readlen(const char *who, uint32_t readlen)
{
    if (readlen >= 1 && readlen <= MT_MAX_LEN) return HARC_AMD_OK;
    harc_set_error("%s: a read length of %u is not 1 .. %u", who, readlen, MT_MAX_LEN);
    return HARC_AMD_EINVAL;
}

extern "C" int harc_amd_motifs_check_host(const void *list, uint64_t list_bytes, uint32_t K, uint64_t *n_motifs)
{
    if (!n_motifs || (list_bytes && !list)) { harc_set_error("motifs_check_host: bad arguments"); return HARC_AMD_EINVAL; }
    std::vector<std::string> motifs;
    *n_motifs = 0;
    RC_TRY(mt_parse_list("motifs_check_host", list, list_bytes, K, &motifs));
    *n_motifs = motifs.size();
    return HARC_AMD_OK;
}

extern "C" int harc_amd_motif_flags_host(const void *list, uint64_t list_bytes, uint32_t K, const void *dna, uint64_t n_lines, uint32_t readlen, uint8_t *flags, uint8_t *hit,
                                         uint64_t *n_motifs, uint64_t *n_found)
{
    if (!n_motifs || !n_found || (list_bytes && !list) || (n_lines && (!dna || !flags))) { harc_set_error("motif_flags_host: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(mt_refuse_readlen("motif_flags_host", readlen));
    std::vector<std::string> motifs;
    RC_TRY(mt_parse_list("motif_flags_host", list, list_bytes, K, &motifs));
    std::vector<uint8_t> h(motifs.size(), 0);
    mt_flags_host(motifs, K, (const uint8_t *)dna, n_lines, readlen, flags, h.data());
    *n_motifs = motifs.size(); *n_found = 0;
    for (size_t k = 0; k < h.size(); k++) { *n_found += h[k]; if (hit) hit[k] = h[k]; }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_motif_flags_device(harc_amd_ctx *c, const void *list, uint64_t list_bytes, uint32_t K, const void *d_dna, uint64_t n_lines, uint32_t readlen,
                                           uint8_t *d_flags, uint8_t *hit, uint64_t *n_motifs, uint64_t *n_found)
{
    if (!c || !n_motifs || !n_found || (list_bytes && !list) || (n_lines && (!d_dna || !d_flags))) { harc_set_error("motif_flags_device: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(mt_refuse_readlen("motif_flags_device", readlen));
    MtSet S; S.K = K;
    RC_TRY(mt_parse_list("motif_flags_device", list, list_bytes, K, &S.motifs));
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    RC_TRY(mt_load_set(c, &S));
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    RC_TRY(mt_launch(c, S, (const char *)d_dna, n_lines, readlen, d_flags));
    RC_TRY(timer.end(c->stream));
    std::vector<uint8_t> h; uint64_t found = 0;
    RC_TRY(mt_hits(c, S, &h, &found));
    if (hit) memcpy(hit, h.data(), h.size());
    const uint64_t bytes = n_lines * ((uint64_t)readlen + 1);
    if (trace) fprintf(stderr, "[match] device call: %llu reads of %u, %llu motifs, K = %u, match kernel %.3f ms (%.1f GB/s of reads)\n", (unsigned long long)n_lines, readlen,
                       (unsigned long long)S.motifs.size(), K, 1e3 * seconds, seconds > 0 ? 1e-9 * (double)bytes / seconds : 0.0);
    *n_motifs = S.motifs.size(); *n_found = found;
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the files
extern "C" int harc_amd_match_files(const harc_amd_params *params, const char *motifs_path, uint32_t K, const char *dna_path, const char *ids_path, const char *quality_path,
                                    const char *out_dna_path, const char *out_ids_path, const char *out_quality_path, uint64_t pair_records, int32_t pair_rule,
                                    uint64_t stats[4], char *missing, uint64_t missing_cap)
{
    if (!params || !motifs_path || !dna_path || !out_dna_path || !stats) { harc_set_error("match_files: bad arguments"); return HARC_AMD_EINVAL; }
    const bool with_q = ids_path != nullptr;
    if (with_q != (quality_path != nullptr) || (with_q && (!out_ids_path || !out_quality_path))) { harc_set_error("match_files: the id file and the quality file come together, each with its output"); return HARC_AMD_EINVAL; }
    if (pair_records && !with_q) { harc_set_error("match_files: a pair is two FASTQ files: without the id and quality files the reads are filtered line by line"); return HARC_AMD_EINVAL; }
    if (pair_records && (pair_rule < IDM_NONE || pair_rule > IDM_SPACE)) { harc_set_error("match_files: %d is no mate rule (0 none, 1 same, 2 slash, 3 space)", (int)pair_rule); return HARC_AMD_EINVAL; }
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (missing && missing_cap) missing[0] = 0;
    uint64_t msz = 0, isz = 0, dsz = 0, qsz = 0;
    if (!file_size(motifs_path, &msz)) { harc_set_error("cannot open %s", motifs_path); return HARC_AMD_EIO; }
    if (!file_size(dna_path, &dsz)) { harc_set_error("cannot open %s", dna_path); return HARC_AMD_EIO; }
    if (with_q && !file_size(ids_path, &isz)) { harc_set_error("cannot open %s", ids_path); return HARC_AMD_EIO; }
    if (with_q && !file_size(quality_path, &qsz)) { harc_set_error("cannot open %s", quality_path); return HARC_AMD_EIO; }
    if (msz > MT_MAX_LIST) { harc_set_error("match_files: the list of motifs %s holds %llu bytes, more than %llu", motifs_path, (unsigned long long)msz, (unsigned long long)MT_MAX_LIST); return HARC_AMD_EINVAL; }
    if (!msz) { harc_set_error("match_files: the list of motifs %s is empty", motifs_path); return HARC_AMD_EINVAL; }
    std::vector<uint8_t> list;
    if (!slurp_file(std::string(motifs_path), list, true)) return HARC_AMD_EIO;
    MtSet set; set.K = K;
    RC_TRY(mt_parse_list("match_files", list.data(), list.size(), K, &set.motifs));
    uint32_t L = 0;
    RC_TRY(first_line_length(dna_path, "match_files", &L));
    const uint64_t S = (uint64_t)L + 1;
    if (dsz % S) { harc_set_error("match_files: the %llu bytes of %s are not lines of %u", (unsigned long long)dsz, dna_path, L); return HARC_AMD_EINVAL; }
    if (with_q && qsz != dsz) { harc_set_error("match_files: %s holds %llu bytes, %s %llu: a quality line per read is wanted", quality_path, (unsigned long long)qsz, dna_path, (unsigned long long)dsz); return HARC_AMD_EINVAL; }
    const uint64_t reads = dsz / S;
    if (reads > 0xFFFFFFFEull) { harc_set_error("match_files: %llu reads are more than one job holds", (unsigned long long)reads); return HARC_AMD_EINVAL; }
    const bool pair = pair_records != 0, once = pair && pair_rule != IDM_NONE;      // once: the id file holds file 1's ids alone
    if (pair && reads != 2 * pair_records) { harc_set_error("match_files: a pair of %llu records is wanted, %s holds %llu reads, not twice as many", (unsigned long long)pair_records, dna_path, (unsigned long long)reads); return HARC_AMD_EINVAL; }
    const uint64_t want_ids = once ? pair_records : reads, per_file = pair ? pair_records : reads;

    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    harc_amd_ctx *c = guard.c;
    const uint64_t big = isz > dsz ? isz : dsz;
    RingGeom g[2];                                                // a feeder and a drain are alive together
    RC_TRY(ring_split(c, 2, 8, "match", g, ring_slice_for(big, 8)));
    LapTimer lap{ "[match]" };
    PoolScope scope(c);
    RC_TRY(mt_load_set(c, &set));
    DevBuf flags{ c };
    RC_TRY(dev_reserve(&flags, (size_t)reads + 1));
    HIP_TRY(hipMemsetAsync(flags.p, 0, (size_t)reads + 1, c->stream));
    lap.lap("list and table");

    // ---- phase A: the flags of the whole job, one byte a line, from the reads in pieces of whole lines
    uint64_t ML = env_u64("HARC_AMD_MATCH_LINES", ((uint64_t)256 << 20) / S);
    if (ML * S > 0x7FFFFFFFull) ML = 0x7FFFFFFFull / S;
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double match_s = 0;
    {
        KernelTimer timer(trace ? &match_s : nullptr);
        DevBuf txt{ c };
        RC_TRY(dev_reserve(&txt, (size_t)((reads < ML ? reads : ML) * S)));
        const Pieces pieces = line_pieces(reads, S, ML);
        FileFeeder feed(c, dna_path);
        RC_TRY(feed.start(pieces, g[0]));
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t bytes = pieces[p].second - pieces[p].first, line0 = pieces[p].first / S;
            RC_TRY(feed.upload_piece(p, txt.p, nullptr));
            RC_TRY(timer.begin(c->stream));
            RC_TRY(mt_launch(c, set, txt.p, bytes / S, L, (uint8_t *)flags.p + line0));
            RC_TRY(timer.end_mark(c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));             // txt is written again by the next piece's upload
            RC_TRY(timer.end_wait());
        }
    }
    if (pair) RC_TRY(harc_flags_or_halves(c, (uint8_t *)flags.p, per_file));      // a pair is selected when either mate matches
    std::vector<uint8_t> h; uint64_t found = 0, selected = 0;
    RC_TRY(mt_hits(c, set, &h, &found));
    RC_TRY(harc_flags_count(c, (const uint8_t *)flags.p, per_file, &selected));
    stats[0] = set.motifs.size(); stats[1] = found; stats[2] = selected; stats[3] = per_file;
    if (trace) fprintf(stderr, "[match] %llu reads of %u matched in %.3f ms of kernels, %llu of %llu motifs found, %llu of %llu records selected\n", (unsigned long long)reads, L, 1e3 * match_s,
                       (unsigned long long)found, (unsigned long long)set.motifs.size(), (unsigned long long)selected, (unsigned long long)per_file);
    if (missing && missing_cap) {
        uint64_t w = 0; int shown = 0;
        for (size_t k = 0; k < h.size() && shown < 10; k++) {
            if (h[k]) continue;
            if (w + set.motifs[k].size() + 2 > missing_cap) break;
            memcpy(missing + w, set.motifs[k].data(), set.motifs[k].size()); w += set.motifs[k].size(); missing[w++] = '\n'; shown++;
        }
        missing[w] = 0;
    }
    lap.lap("phase A");

    // ---- phase B: the gather of -L over the one or three texts
    GatherFiles J;
    J.who = "match_files"; J.ids_path = ids_path; J.dna_path = dna_path; J.quality_path = quality_path;
    J.out_ids_path = out_ids_path; J.out_dna_path = out_dna_path; J.out_quality_path = out_quality_path;
    J.isz = isz; J.id_lines = want_ids; J.ids_counted = false; J.reads = reads; J.S = S; J.out_lines = pair ? 2 * selected : selected; J.flags = (const uint8_t *)flags.p;
    J.feed = g[0]; J.drain = g[1]; J.lap = &lap;
    return harc_gather_files(c, J);
}
