// qmap.hip -- lossy quality values on the device (./harc -c -q -b SPEC; README: "-b and what it promises").  Every rule, and the body of both kernels as a function of
// a lane number, is qm_block.h's; this file gives the bodies their lanes, reduces what the lanes counted, and holds the calls of the C-ABI.
//   k_qm_table    a table scheme as one streaming pass, 16 bytes a lane and iteration, the 256-byte table in LDS (64 dwords, one per bank).  The statistics are a
//                 template flag: without them no register and no instruction is theirs.  With them every lane counts in registers (sums, a maximum, two 64-bit
//                 presence masks each for the values before and after), a wave reduces them by shuffles, and one lane adds them with one atomic per number.
//   k_qm_pblock   run smoothing: a workgroup of 256 per tile of 256 lines -- the tile comes into LDS rows of an odd number of dwords by aligned 16-byte loads, lane t
//                 walks row t (the cut is serial along a line), and the tile leaves by aligned 16-byte stores.  256 rows of up to 65 dwords: 66 560 bytes at most.
// Both work in place (d_out == d_text) and out of place; the stride check of the text rides along in both (qm_block.h) and is reported in qpack's words.
#include "devutil.h"
#include "qm_block.h"
#include "fileio.h"
#include <string>

#define QM_T 256
#define QM_SLOTS 10                                               // the eight numbers of a QmAcc and the two of the stride check

struct QmTable { uint8_t t[256]; };

__device__ __forceinline__ uint64_t qm_wave_sum(uint64_t v) { for (int o = 32; o > 0; o >>= 1) v += shfl_u64_any(v, o); return v; }
__device__ __forceinline__ uint64_t qm_wave_or(uint64_t v) { for (int o = 32; o > 0; o >>= 1) v |= shfl_u64_any(v, o); return v; }
__device__ __forceinline__ uint64_t qm_wave_max(uint64_t v) { for (int o = 32; o > 0; o >>= 1) { const uint64_t w = shfl_u64_any(v, o); v = w > v ? w : v; } return v; }
// what the lanes of a wave counted -> slots[0 .. 8) (STATS) and slots[8 .. 10), one atomic per number that is not zero
template <bool STATS> __device__ __forceinline__ void qm_wave_flush(const QmAcc &a, const uint64_t *err, unsigned long long *slots)
{
    const bool first = (threadIdx.x & 63u) == 0;
    if (STATS) {
        const uint64_t changed = qm_wave_sum(a.changed), sum_abs = qm_wave_sum(a.sum_abs), sum_sq = qm_wave_sum(a.sum_sq), max_abs = qm_wave_max(a.max_abs);
        const uint64_t in_lo = qm_wave_or(a.in_lo), in_hi = qm_wave_or(a.in_hi), out_lo = qm_wave_or(a.out_lo), out_hi = qm_wave_or(a.out_hi);
        if (first) {
            if (changed) atomicAdd(&slots[0], (unsigned long long)changed);
            if (sum_abs) atomicAdd(&slots[1], (unsigned long long)sum_abs);
            if (sum_sq) atomicAdd(&slots[2], (unsigned long long)sum_sq);
            if (in_lo) atomicOr(&slots[3], (unsigned long long)in_lo);
            if (in_hi) atomicOr(&slots[4], (unsigned long long)in_hi);
            if (out_lo) atomicOr(&slots[5], (unsigned long long)out_lo);
            if (out_hi) atomicOr(&slots[6], (unsigned long long)out_hi);
            if (max_abs) atomicMax(&slots[7], (unsigned long long)max_abs);
        }
    }
    const uint64_t e0 = qm_wave_sum(err[0]), e1 = qm_wave_sum(err[1]);
    if (first) {
        if (e0) atomicAdd(&slots[8], (unsigned long long)e0);
        if (e1) atomicAdd(&slots[9], (unsigned long long)e1);
    }
}

// slots[8]: newlines on the stride, slots[9]: newlines in all
template <bool STATS> __global__ __launch_bounds__(QM_T) void k_qm_table(const uint8_t *in, uint8_t *out, uint64_t N, uint32_t L, QmTable tab, unsigned long long *slots)
{
    __shared__ __attribute__((aligned(16))) uint8_t table[256];
    table[threadIdx.x] = tab.t[threadIdx.x];
    __syncthreads();
    QmAcc acc; qm_acc_zero(&acc);
    uint64_t err[2] = { 0, 0 };
    qm_table_item<STATS>(in, out, N, L, table, (uint64_t)blockIdx.x * QM_T + threadIdx.x, (uint64_t)gridDim.x * QM_T, &acc, err);
    qm_wave_flush<STATS>(acc, err, slots);
}

// slots[8]: stride positions without a newline, slots[9]: newlines inside a line
template <bool STATS> __global__ __launch_bounds__(QM_T) void k_qm_pblock(const uint8_t *in, uint8_t *out, uint64_t n_lines, uint32_t L, uint32_t R, uint64_t ntiles, unsigned long long *slots)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t qm_rows[];
    const uint64_t b = harc_bid();
    if (b >= ntiles) return;
    const uint32_t t = threadIdx.x, LL = L + 1u, pitch = 4u * qm_pitch(L);
    const uint64_t line0 = b * (uint64_t)QM_TILE;
    const uint32_t m = n_lines - line0 < QM_TILE ? (uint32_t)(n_lines - line0) : QM_TILE, T = m * LL;
    qm_tile_load(in + line0 * LL, T, LL, pitch, qm_rows, t, QM_T);
    __syncthreads();
    QmAcc acc; qm_acc_zero(&acc);
    uint64_t err[2] = { 0, 0 };
    qm_tile_walk<STATS>(qm_rows, m, L, pitch, R, t, &acc, err);
    __syncthreads();
    qm_tile_store(out + line0 * LL, T, LL, pitch, qm_rows, t, QM_T);
    qm_wave_flush<STATS>(acc, err, slots);
}

// ------------------------------------------------------------------------------------------------ the map itself: valid, or refused by name
int harc_qmap_check(const char *who, const harc_amd_qmap *map)
{
    if (!map) { harc_set_error("%s: no map", who); return HARC_AMD_EINVAL; }
    if (map->kind == QM_KIND_TABLE) {
        const int bad = qm_table_bad(map->table);
        if (bad < 0) return HARC_AMD_OK;
        if (qm_is_value((uint32_t)bad)) harc_set_error("%s: the table maps the byte value %d to %d, outside 33..126", who, bad, (int)map->table[bad]);
        else harc_set_error("%s: the table changes the byte value %d (to %d): only 33..126 may change", who, bad, (int)map->table[bad]);
        return HARC_AMD_EINVAL;
    }
    if (map->kind == QM_KIND_PBLOCK) {
        if (map->radius >= 1 && map->radius <= (int32_t)QM_MAXR) return HARC_AMD_OK;
        harc_set_error("%s: the radius %d of the run smoothing is not in 1..%u", who, map->radius, QM_MAXR);
        return HARC_AMD_EINVAL;
    }
    harc_set_error("%s: the kind %d of the map is neither 1 (a table) nor 2 (run smoothing)", who, map->kind);
    return HARC_AMD_EINVAL;
}
static int qm_refuse_stride(uint32_t L, uint64_t e0, uint64_t e1)
{
    harc_set_error("qpack: the text is not lines of %u quality values: %llu positions on the %u-byte stride hold no newline and %llu newlines are off it", L, (unsigned long long)e0, L + 1,
                   (unsigned long long)e1);
    return HARC_AMD_EINVAL;
}

// n lines of L at d_text -> d_out (the same pointer, or disjoint), map checked by the caller.  acc (may be null): what the mapping did is added to it; seconds
// (may be null): the kernel's are added
int harc_qmap_run(harc_amd_ctx *c, const char *d_text, uint64_t n, uint32_t L, const harc_amd_qmap *map, char *d_out, QmAcc *acc, double *seconds)
{
    if (!n) return HARC_AMD_OK;
    const uint64_t N = n * (L + 1ull);
    PoolScope scope(c);
    unsigned long long *slots = nullptr;
    RC_TRY(dalloc(c, &slots, QM_SLOTS));
    HIP_TRY(hipMemsetAsync(slots, 0, 8 * QM_SLOTS, c->stream));
    KernelTimer timer(seconds);
    RC_TRY(timer.begin(c->stream));
    const uint8_t *in = (const uint8_t *)d_text; uint8_t *out = (uint8_t *)d_out;
    if (map->kind == QM_KIND_TABLE) {
        QmTable tab; memcpy(tab.t, map->table, 256);
        uint64_t blocks = ((N >> 4) + QM_T * 4 - 1) / (QM_T * 4);  // four chunks a lane, up to eight workgroups a CU
        if (blocks < 1) blocks = 1;
        if (blocks > 2048) blocks = 2048;
        if (acc) hipLaunchKernelGGL(k_qm_table<true>, dim3((unsigned)blocks), dim3(QM_T), 0, c->stream, in, out, N, L, tab, slots);
        else hipLaunchKernelGGL(k_qm_table<false>, dim3((unsigned)blocks), dim3(QM_T), 0, c->stream, in, out, N, L, tab, slots);
    } else {
        const uint64_t ntiles = (n + QM_TILE - 1) / QM_TILE;
        const uint32_t lds = QM_TILE * 4u * qm_pitch(L);
        if (acc) hipLaunchKernelGGL(k_qm_pblock<true>, harc_fold256(ntiles), dim3(QM_T), lds, c->stream, in, out, n, L, (uint32_t)map->radius, ntiles, slots);
        else hipLaunchKernelGGL(k_qm_pblock<false>, harc_fold256(ntiles), dim3(QM_T), lds, c->stream, in, out, n, L, (uint32_t)map->radius, ntiles, slots);
    }
    HIP_TRY(hipGetLastError());
    RC_TRY(timer.end_mark(c->stream));
    unsigned long long h[QM_SLOTS];
    HIP_TRY(hipMemcpyAsync(h, slots, 8 * QM_SLOTS, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    RC_TRY(timer.end_wait());
    const uint64_t e0 = map->kind == QM_KIND_TABLE ? n - h[8] : h[8], e1 = map->kind == QM_KIND_TABLE ? h[9] - h[8] : h[9];
    if (e0 || e1) return qm_refuse_stride(L, e0, e1);
    if (acc) { QmAcc a = { h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7] }; qm_acc_merge(acc, &a); }
    return HARC_AMD_OK;
}

static int qm_check_readlen(const char *who, int32_t readlen)
{
    if (readlen < 1 || readlen > 255) { harc_set_error("%s: the read length %d is not in 1..255", who, readlen); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}
static int qm_check_overlap(const char *who, const char *text, const char *out, uint64_t N)
{
    const uintptr_t a = (uintptr_t)text, b = (uintptr_t)out;
    if (a != b && a < b + N && b < a + N) { harc_set_error("%s: the output overlaps the text without being the text: in place, or apart", who); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_qmap_device(harc_amd_ctx *c, const char *d_text, uint64_t n_reads, int32_t readlen, const harc_amd_qmap *map, char *d_out, harc_amd_qmap_stats *stats)
{
    if (!c || (n_reads && (!d_text || !d_out))) { harc_set_error("qmap_device: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(qm_check_readlen("qmap_device", readlen));
    RC_TRY(harc_qmap_check("qmap_device", map));
    RC_TRY(qm_check_overlap("qmap_device", d_text, d_out, n_reads * (readlen + 1ull)));
    HIP_TRY(hipSetDevice(c->P.device));
    QmAcc acc; qm_acc_zero(&acc);
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    RC_TRY(harc_qmap_run(c, d_text, n_reads, (uint32_t)readlen, map, d_out, stats ? &acc : nullptr, trace ? &seconds : nullptr));
    if (stats) qm_acc_stats(&acc, n_reads * (uint64_t)readlen, stats);
    if (trace) fprintf(stderr, "[qmap] device call: %llu bytes of text, kernel %.3f ms (%.1f GB/s of text)\n", (unsigned long long)(n_reads * (readlen + 1ull)), 1e3 * seconds,
                       seconds > 0 ? 1e-9 * (double)(n_reads * (readlen + 1ull)) / seconds : 0.0);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_qmap_host(const char *text, uint64_t n_reads, int32_t readlen, const harc_amd_qmap *map, char *out, harc_amd_qmap_stats *stats)
{
    if (n_reads && (!text || !out)) { harc_set_error("qmap_host: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(qm_check_readlen("qmap_host", readlen));
    RC_TRY(harc_qmap_check("qmap_host", map));
    RC_TRY(qm_check_overlap("qmap_host", text, out, n_reads * (readlen + 1ull)));
    QmAcc acc; qm_acc_zero(&acc);
    uint64_t err[2] = { 0, 0 };
    if (stats) qm_map_text<true>((const uint8_t *)text, n_reads, (uint32_t)readlen, map, (uint8_t *)out, &acc, err);
    else qm_map_text<false>((const uint8_t *)text, n_reads, (uint32_t)readlen, map, (uint8_t *)out, &acc, err);
    if (err[0] || err[1]) return qm_refuse_stride((uint32_t)readlen, err[0], err[1]);
    if (stats) qm_acc_stats(&acc, n_reads * (uint64_t)readlen, stats);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the spec strings
// the decimal number at *p, digits only and at most four of them -> *v, *p behind it; 0: none there
static int qm_number(const char **p, long *v)
{
    const char *q = *p; long x = 0; int nd = 0;
    while (*q >= '0' && *q <= '9' && nd < 5) { x = x * 10 + (*q - '0'); q++; nd++; }
    if (nd == 0 || nd > 4) return 0;
    *v = x; *p = q;
    return 1;
}
// `nf` fields ":<number>" behind the name at p, named names[k] and held to lo[k] .. hi[k]
static int qm_fields(const char *spec, const char *p, int nf, const char *const *names, const long *lo, const long *hi, long *v)
{
    for (int k = 0; k < nf; k++) {
        if (*p != ':') { harc_set_error("qmap_parse: '%s': the field %s is missing", spec, names[k]); return HARC_AMD_EINVAL; }
        p++;
        if (!qm_number(&p, &v[k])) { harc_set_error("qmap_parse: '%s': the field %s is no number of one to four digits", spec, names[k]); return HARC_AMD_EINVAL; }
        if (*p && *p != ':' && k + 1 < nf) { harc_set_error("qmap_parse: '%s': the field %s has the character '%c' in it: digits only", spec, names[k], *p); return HARC_AMD_EINVAL; }
        if (v[k] < lo[k] || v[k] > hi[k]) { harc_set_error("qmap_parse: '%s': the field %s = %ld is not in %ld..%ld", spec, names[k], v[k], lo[k], hi[k]); return HARC_AMD_EINVAL; }
    }
    if (*p == ':' && !nf) { harc_set_error("qmap_parse: '%s': a field behind the name of a scheme that takes none", spec); return HARC_AMD_EINVAL; }
    if (*p == ':') { harc_set_error("qmap_parse: '%s': a field behind %s, the last that the scheme takes", spec, names[nf - 1]); return HARC_AMD_EINVAL; }
    if (*p) { harc_set_error("qmap_parse: '%s': trailing characters '%s' behind %s", spec, p, nf ? names[nf - 1] : "the name"); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_qmap_parse(const char *spec, harc_amd_qmap *out)
{
    if (!spec || !out) { harc_set_error("qmap_parse: bad arguments"); return HARC_AMD_EINVAL; }
    size_t nn = 0;
    while (spec[nn] && spec[nn] != ':') nn++;
    const std::string name(spec, nn);
    harc_amd_qmap m; memset(&m, 0, sizeof m);
    for (int v = 0; v < 256; v++) m.table[v] = (uint8_t)v;
    long v[3] = { 0, 0, 0 };
    if (name == "ill8") {
        RC_TRY(qm_fields(spec, spec + nn, 0, nullptr, nullptr, nullptr, v));
        m.kind = QM_KIND_TABLE; qm_fill_table(m.table, 0, 0, 0, 0);
    } else if (name == "bin") {
        static const char *const names[3] = { "T", "H", "L" };
        static const long lo[3] = { 1, 0, 0 }, hi[3] = { 93, 93, 93 };
        RC_TRY(qm_fields(spec, spec + nn, 3, names, lo, hi, v));
        if (v[2] > v[1]) { harc_set_error("qmap_parse: '%s': the field L = %ld is above H = %ld", spec, v[2], v[1]); return HARC_AMD_EINVAL; }
        m.kind = QM_KIND_TABLE; qm_fill_table(m.table, 1, (uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
    } else if (name == "cap") {
        static const char *const names[1] = { "M" };
        static const long lo[1] = { 0 }, hi[1] = { 93 };
        RC_TRY(qm_fields(spec, spec + nn, 1, names, lo, hi, v));
        m.kind = QM_KIND_TABLE; qm_fill_table(m.table, 2, (uint32_t)v[0], 0, 0);
    } else if (name == "pblock") {
        static const char *const names[1] = { "R" };
        static const long lo[1] = { 1 }, hi[1] = { (long)QM_MAXR };
        RC_TRY(qm_fields(spec, spec + nn, 1, names, lo, hi, v));
        m.kind = QM_KIND_PBLOCK; m.radius = (int32_t)v[0];
    } else {
        harc_set_error("qmap_parse: '%s': the name '%s' is none of ill8, bin, cap and pblock", spec, name.c_str());
        return HARC_AMD_EINVAL;
    }
    *out = m;
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the file
extern "C" int harc_amd_qmap_files(const harc_amd_params *params, const char *quality_path, const char *out_path, const harc_amd_qmap *map, harc_amd_qmap_stats *stats)
{
    if (!params || !quality_path || !out_path) { harc_set_error("qmap_files: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(harc_qmap_check("qmap_files", map));
    uint64_t qsz = 0;
    if (!file_size(quality_path, &qsz)) { harc_set_error("cannot open %s", quality_path); return HARC_AMD_EIO; }
    {   // the same file under two names must not be opened for writing: the refusal comes before the guard that removes the output
        struct stat a, b;
        if (!strcmp(quality_path, out_path) || (stat(quality_path, &a) == 0 && stat(out_path, &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)) {
            harc_set_error("qmap_files: the output %s is the input: the mapped file needs a name of its own", out_path); return HARC_AMD_EINVAL; }
    }
    OutFileGuard outguard{ out_path };
    uint32_t L = 1;
    if (qsz) RC_TRY(first_line_length(quality_path, "qmap_files", &L));
    const uint64_t LL = L + 1ull;
    if (qsz % LL) { harc_set_error("qmap_files: %s holds %llu bytes, no multiple of the %llu bytes of a line of %u quality values and its newline", quality_path, (unsigned long long)qsz, (unsigned long long)LL, L); return HARC_AMD_EINVAL; }
    const uint64_t n = qsz / LL;
    const uint64_t dflt = ((uint64_t)64 << 20) / LL, piece_lines = env_u64("HARC_AMD_QMAP_PIECE", dflt ? dflt : 1);
    CtxGuard guard;
    RC_TRY(side_context(params, (int)L, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom g[2];                                                // the feeder's and the drain's
    RC_TRY(ring_split(c, 2, 8, "quality", g));
    DevBuf txt{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0, t_kernel = 0;
    QmAcc acc; qm_acc_zero(&acc);
    int npieces = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)qsz, &g[1], true));
        const Pieces pieces = line_pieces(n, LL, piece_lines);
        FileFeeder feed(c, quality_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, g[0]));
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t bytes = pieces[p].second - pieces[p].first, m = bytes / LL;
            RC_TRY(dev_reserve(&txt, (size_t)bytes));
            { const double t0 = mono_now(); RC_TRY(feed.upload_piece(p, txt.p, nullptr)); t_read += mono_now() - t0; }
            RC_TRY(harc_qmap_run(c, txt.p, m, L, map, txt.p, stats ? &acc : nullptr, tlog ? &t_kernel : nullptr));
            { const double t0 = mono_now(); RC_TRY(drain.put(txt.p, (size_t)bytes, pieces[p].first)); t_write += mono_now() - t0; }
            npieces++;
        }
        drain.set_final_size(qsz);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    if (stats) qm_acc_stats(&acc, n * (uint64_t)L, stats);
    if (tlog) fprintf(stderr, "[qmap] %llu bytes of text in %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers\n", (unsigned long long)qsz, npieces,
                      t_kernel, t_read, t_write);
    outguard.ok = true;
    return HARC_AMD_OK;
}
