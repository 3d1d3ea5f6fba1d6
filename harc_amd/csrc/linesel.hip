// linesel.hip -- where line k of a text starts, found on the GPU (./harc -d -r; README: "-r and what it promises").  The arithmetic is linesel.h's.
//   k_ls_count    one streaming read, as k_text_digest of check.hip: aligned 16-byte loads over the 16-byte hull of the text, a lane masks the bytes of the first
//                 and the last chunk that are not the text's, a newline mask and its popcount per chunk, a reduction across the wave, one count per workgroup.
//                 A workgroup owns a span of consecutive rows of LS_T chunks.
//   (the library's exclusive scan over the counts)
//   k_ls_select   the one workgroup whose span holds the k-th newline walks its span again, row by row: the counts of the lanes are scanned across the wave,
//                 a ballot names the lane whose chunk holds the newline, the lane picks the bit.  Every other workgroup leaves at once.
// No atomics: the answer is a function of the text.
#include "devutil.h"
#include "linesel.h"
#include "fileio.h"

#define LS_T 256
#define LS_WAVES (LS_T / 64)

// the newlines of chunk k of the hull, those of bytes outside the text masked off; 0 for a chunk past the hull
__device__ __forceinline__ uint32_t ls_chunk_mask(const uint4 *base, uint64_t k, uint64_t nchunks, uint64_t mis, uint64_t hull)
{
    if (k >= nchunks) return 0;
    const uint4 v = base[k];
    const uint32_t m = ls_newline_bits(v.x) | (ls_newline_bits(v.y) << 4) | (ls_newline_bits(v.z) << 8) | (ls_newline_bits(v.w) << 12);
    return m & ls_keep_bits(k << 4, mis, hull);
}
__device__ __forceinline__ uint32_t ls_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// workgroup b: the newlines of rows [b * rows, (b + 1) * rows) of LS_T chunks -> cnt[b]
__global__ __launch_bounds__(LS_T) void k_ls_count(const uint8_t *p, uint64_t n, uint64_t rows, uint32_t *cnt)
{
    __shared__ uint32_t part[LS_WAVES];
    const uint64_t mis = (uint64_t)((uintptr_t)p & 15u), hull = mis + n, nchunks = (hull + 15) >> 4;
    const uint4 *base = (const uint4 *)(p - mis);
    const uint64_t c0 = (uint64_t)blockIdx.x * rows * LS_T + threadIdx.x;
    uint32_t nl = 0;
#pragma unroll 4
    for (uint64_t r = 0; r < rows; r++) nl += (uint32_t)__popc(ls_chunk_mask(base, c0 + r * LS_T, nchunks, mis, hull));
    nl = ls_wave_sum(nl);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = nl;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t s = 0; for (int w = 0; w < LS_WAVES; w++) s += part[w]; cnt[blockIdx.x] = s; }
}

// before[b]: the newlines in front of workgroup b's span, before[gridDim.x]: all of them.  out[0] = the newlines, out[1] = where line k starts
__global__ __launch_bounds__(LS_T) void k_ls_select(const uint8_t *p, uint64_t n, uint64_t rows, const uint32_t *before, uint64_t k, unsigned long long *out)
{
    __shared__ uint32_t part[LS_WAVES];
    const uint32_t lo = before[blockIdx.x], hi = before[blockIdx.x + 1], total = before[gridDim.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[0] = total;
        if (k == 0) out[1] = 0; else if (k > (uint64_t)total) out[1] = LS_NONE;
    }
    if (k <= (uint64_t)lo || k > (uint64_t)hi) return;            // (uniform over the workgroup; k == 0 and k > total leave here too)
    const uint64_t mis = (uint64_t)((uintptr_t)p & 15u), hull = mis + n, nchunks = (hull + 15) >> 4;
    const uint4 *base = (const uint4 *)(p - mis);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t want = (uint32_t)(k - lo);                           // the want-th newline of what is left of the span, counted from 1
    for (uint64_t r = 0; r < rows; r++) {
        const uint64_t chunk = ((uint64_t)blockIdx.x * rows + r) * LS_T + threadIdx.x;
        const uint32_t m = ls_chunk_mask(base, chunk, nchunks, mis, hull), c = (uint32_t)__popc(m);
        uint32_t incl = c;                                        // the newlines of lanes 0 .. lane of this wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += o; }
        if (lane == 63u) part[wave] = incl;
        __syncthreads();
        uint32_t front = 0, row = 0;                              // the newlines of the waves in front of this one, of the whole row
        for (uint32_t w = 0; w < LS_WAVES; w++) { if (w < wave) front += part[w]; row += part[w]; }
        if (want <= row) {
            // the wave whose lanes pass `want`: the first such lane holds the newline
            const unsigned long long reach = __ballot(front < want && front + incl >= want);
            if (reach) {
                const uint32_t first = (uint32_t)__ffsll((long long)reach) - 1u;
                if (lane == first) out[1] = (chunk << 4) + ls_nth_bit(m, want - front - (incl - c)) - mis + 1;
            }
            return;
        }
        want -= row;
        __syncthreads();                                          // part[] is written again
    }
}

struct LsGeom { uint64_t rows; uint32_t blocks; };
static LsGeom ls_geom(uint64_t n)
{
    const uint64_t nchunks = (n + 15 + 15) >> 4, nrows = (nchunks + LS_T - 1) / LS_T;      // at most: the hull of a text that starts at byte 15 of a chunk
    uint64_t blocks = (nrows + 3) / 4;                            // four chunks a lane at least, up to eight workgroups a CU
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    const uint64_t rows = (nrows + blocks - 1) / blocks;
    return LsGeom{ rows ? rows : 1, (uint32_t)blocks };
}

extern "C" int harc_amd_line_offset_device(harc_amd_ctx *c, const void *d_text, uint64_t nbytes, uint64_t k, uint64_t out[2])
{
    if (!c || !out || (nbytes && !d_text)) { harc_set_error("line_offset_device: bad arguments"); return HARC_AMD_EINVAL; }
    if (nbytes > 0xFFFFFFFFull) { harc_set_error("line_offset_device: %llu bytes are more than the 2^32 - 1 of one call (a longer text goes in pieces: harc_amd_line_range_files)", (unsigned long long)nbytes); return HARC_AMD_EINVAL; }
    out[0] = 0; out[1] = k == 0 ? 0 : LS_NONE;
    if (!nbytes) return HARC_AMD_OK;
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    const LsGeom g = ls_geom(nbytes);
    uint32_t *cnt = nullptr, *before = nullptr; unsigned long long *d_out = nullptr;
    RC_TRY(dalloc(c, &cnt, (size_t)g.blocks + 1)); RC_TRY(dalloc(c, &before, (size_t)g.blocks + 1)); RC_TRY(dalloc(c, &d_out, 2));
    HIP_TRY(hipMemsetAsync(cnt + g.blocks, 0, 4, c->stream));
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    hipLaunchKernelGGL(k_ls_count, dim3(g.blocks), dim3(LS_T), 0, c->stream, (const uint8_t *)d_text, nbytes, g.rows, cnt);
    HIP_TRY(hipGetLastError());
    RC_TRY(prim_excl_scan_u32(c, cnt, before, (size_t)g.blocks + 1));
    hipLaunchKernelGGL(k_ls_select, dim3(g.blocks), dim3(LS_T), 0, c->stream, (const uint8_t *)d_text, nbytes, g.rows, (const uint32_t *)before, k, d_out);
    HIP_TRY(hipGetLastError());
    RC_TRY(timer.end_mark(c->stream));
    unsigned long long h[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(h, d_out, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    RC_TRY(timer.end_wait());
    out[0] = h[0]; out[1] = h[1];
    if (trace) fprintf(stderr, "[linesel] device call: %llu bytes of text, line %llu of %llu, kernels %.3f ms (%.1f GB/s of text)\n", (unsigned long long)nbytes, (unsigned long long)k,
                       (unsigned long long)h[0], 1e3 * seconds, seconds > 0 ? 1e-9 * (double)nbytes / seconds : 0.0);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_line_offset_host(const void *text, uint64_t nbytes, uint64_t k, uint64_t out[2])
{
    if (!out || (nbytes && !text)) { harc_set_error("line_offset_host: bad arguments"); return HARC_AMD_EINVAL; }
    ls_line_offset_host((const uint8_t *)text, nbytes, k, out);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the file
extern "C" int harc_amd_line_range_files(const harc_amd_params *params, const char *path, uint64_t first_line, uint64_t n_lines, uint64_t out[2])
{
    if (!params || !path || !out) { harc_set_error("line_range_files: bad arguments"); return HARC_AMD_EINVAL; }
    if (n_lines > ~first_line) { harc_set_error("line_range_files: lines %llu + %llu pass 2^64", (unsigned long long)first_line, (unsigned long long)n_lines); return HARC_AMD_EINVAL; }
    uint64_t fsz = 0;
    if (!file_size(path, &fsz)) { harc_set_error("cannot open %s", path); return HARC_AMD_EIO; }
    const uint64_t last = first_line + n_lines;                   // the range ends where line `last` starts
    uint64_t begin = first_line == 0 ? 0 : LS_NONE, end = last == 0 ? 0 : LS_NONE, seen = 0;
    if (fsz && end == LS_NONE) {
        uint64_t piece = env_u64("HARC_AMD_LINESEL_PIECE", (uint64_t)256 << 20);
        if (piece > 0xFFFFFFFFull) piece = 0xFFFFFFFFull;
        CtxGuard guard;
        RC_TRY(side_context(params, 100, &guard.c));
        harc_amd_ctx *c = guard.c;
        RingGeom g;
        RC_TRY(ring_split(c, 1, 16, "line select", &g, ring_slice_for(fsz < piece ? fsz : piece, 16)));      // a short file or short pieces do not pin a ring of 1 GiB
        const Pieces pieces = byte_pieces(0, fsz, piece);
        DevBuf txt{ c };
        RC_TRY(dev_reserve(&txt, (size_t)(fsz < piece ? fsz : piece)));
        FileFeeder feed(c, path);
        RC_TRY(feed.start(pieces, g));
        // the newlines in front of a piece are carried; a piece is asked for the line that is still looked for, and stops the walk when it holds the end
        for (size_t p = 0; p < pieces.size() && end == LS_NONE; p++) {
            const uint64_t a = pieces[p].first, len = pieces[p].second - a;
            RC_TRY(feed.upload_piece(p, txt.p, nullptr));
            uint64_t r[2] = { 0, 0 };
            if (begin == LS_NONE) {
                RC_TRY(harc_amd_line_offset_device(c, txt.p, len, first_line - seen, r));
                if (r[1] != LS_NONE) begin = a + r[1];
            }
            if (begin != LS_NONE && last - seen >= 1) {
                RC_TRY(harc_amd_line_offset_device(c, txt.p, len, last - seen, r));
                if (r[1] != LS_NONE) end = a + r[1];
            }
            seen += r[0];
        }
    }
    if (n_lines == 0 && begin != LS_NONE) end = begin;
    if (begin == LS_NONE || end == LS_NONE) {
        harc_set_error("line_range_files: lines %llu .. %llu of %s are wanted, it holds %llu lines", (unsigned long long)first_line + 1, (unsigned long long)last, path, (unsigned long long)seen);
        return HARC_AMD_EINVAL;
    }
    out[0] = begin; out[1] = end;
    return HARC_AMD_OK;
}
