// gunzip.hip -- any gzip file (one DEFLATE stream per member) -> its text, inflated in parallel on the device; the rules are inflate_stream.h's.
//   k_gz_find       a wave per chunk of compressed bytes: its 64 lanes test 64 consecutive bit offsets a round for a non-final dynamic block header, the lowest hit wins
//   k_gz_count      a lane per start, in the shape of k_bgzf_inflate (an ImTables slot per lane in global memory): block after block to the end of its chunk, text counted
//   (the chain)     on the host, O(chunks): the walk that starts where the one before ended is next; where none does, one walk is counted from there (a repair)
//   k_gz_write      a lane per walk of the chain: the same walk, 16-bit symbols (a literal, or 0x8000 | index into the unknown window) at the scan of the text counts
//   k_gz_window     one workgroup over the walks in file order: the resolved 32 KiB behind a walk from the resolved 32 KiB in front of it and its symbols
//   k_gz_translate  a workgroup per 16 KiB of text, all walks in parallel: symbols -> bytes (16-byte stores where aligned) and the tile's CRC-32 (64-byte spans
//                   folded with dm_gfmul / dm_xpow8); the host folds the tiles per member and checks CRC-32 and ISIZE against the trailer
// The plan (header, stages 1-3, trailer) and its execution (stages 4-6) are written once over a small backend interface: the device, and the host in a row
// (harc_amd_gunzip_host: what the tests hold the device to, stats included).  harc_amd_gunzip_files feeds pieces of the file through the pinned ring.
#include "devutil.h"
#include "inflate_stream.h"
#include "deflate_member.h"
#include "fileio.h"
#include <memory>
#include <string>
#include <vector>

#define GZ_CHUNK (256u << 10)
#define GZ_TILE 16384u           // text bytes a workgroup translates: 256 spans of 64 bytes
#define GZ_SPAN 64u
#define GZ_PITCH 17u             // dwords of a span's row in LDS: odd, so that 64 lanes walking 64 rows hit 64 banks
#define GZ_SLOTS 65536u          // lanes of the count / write kernels at most
#define GZ_WAVES 1024u           // waves of the finder at most (64 ImTables slots each)
#define GZ_HDR_PEEK 70000u       // bytes looked at for a member header: 10 + 2 + 65535 of FEXTRA and room for names

struct GzRow { uint64_t bit, stop_bit; };                                         // a start (IS_NONE: none) and where its walk may stop
struct GzWalkRow { uint64_t bit, end_bit, text_off, text; uint32_t have, pad; };  // a walk of the chain; have: bytes of window that exist in front of it

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(64) void k_gz_find(const uint8_t *in, uint64_t n, uint64_t base, uint64_t cb, uint64_t k0, uint64_t nk, ImTables *tabs, unsigned long long *cand)
{
    ImTables &t = tabs[(uint64_t)blockIdx.x * 64 + threadIdx.x];
    for (uint64_t i = blockIdx.x; i < nk; i += gridDim.x) {
        const uint64_t lo = (base + (k0 + i) * cb) * 8;
        uint64_t hi = base + (k0 + i + 1) * cb; if (hi > n) hi = n; hi *= 8;
        unsigned long long found = IS_NONE;
        for (uint64_t r = lo; r < hi; r += 64) {                  // the wave stops at the chunk's end
            const uint64_t bit = r + threadIdx.x;
            const bool hit = bit < hi && is_try(in, n, bit, t);
            const unsigned long long m = __ballot(hit);
            if (m) { found = r + (uint64_t)(__ffsll((long long)m) - 1); break; }
        }
        if (threadIdx.x == 0) cand[i] = found;
    }
}
__global__ __launch_bounds__(64) void k_gz_count(const uint8_t *in, uint64_t n, const GzRow *rows, uint32_t nr, ImTables *tabs, uint32_t nslots, IsWalk *res, int32_t *rcs)
{
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= nslots) return;
    ImTables &t = tabs[g];
    for (uint32_t i = g; i < nr; i += nslots) {
        const GzRow r = rows[i];
        IsWalk w; w.end_bit = r.bit; w.text = 0; w.final = 0; w.more = 0;
        rcs[i] = r.bit == IS_NONE ? -1 : is_count(in, n, r.bit, r.stop_bit, t, &w);
        res[i] = w;
    }
}
// the first walk that does not repeat its count (lowest index) ends up in *bad as (index << 8 | code)
__global__ __launch_bounds__(64) void k_gz_write(const uint8_t *in, uint64_t n, const GzWalkRow *rows, uint32_t nw, uint16_t *sym, ImTables *tabs, uint32_t nslots, unsigned long long *bad)
{
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= nslots) return;
    ImTables &t = tabs[g];
    for (uint32_t i = g; i < nw; i += nslots) {
        const GzWalkRow r = rows[i];
        IsWalk w;
        int rc = is_walk(in, n, r.bit, r.end_bit, t, sym + r.text_off, r.text, &w);
        if (!rc && (w.end_bit != r.end_bit || w.text != r.text)) rc = IM_E_SHORT;
        if (rc) atomicMin(bad, ((unsigned long long)i << 8) | (unsigned long long)rc);
    }
}
// wins: nw + 1 windows of IS_WIN bytes, the first given; window w + 1 lies behind walk w
__global__ __launch_bounds__(1024) void k_gz_window(const uint16_t *sym, const GzWalkRow *rows, uint32_t nw, uint8_t *wins)
{
    for (uint32_t w = 0; w < nw; w++) {
        const uint8_t *win = wins + (uint64_t)w * IS_WIN; uint8_t *out = wins + (uint64_t)(w + 1) * IS_WIN;
        const uint16_t *s = sym + rows[w].text_off; const uint64_t T = rows[w].text;
        for (uint32_t j = threadIdx.x; j < IS_WIN; j += 1024) out[j] = is_window_byte(win, s, T, j);
        __syncthreads();
    }
}
// the CRC-32 of a tile of tlen <= GZ_TILE bytes from the CRC-32s of its 64-byte spans, in a row (crc(A B) = crc(A) x^(8 |B|) + crc(B))
IM_HD uint32_t gz_fold_spans(const uint32_t *cc, uint32_t tlen)
{
    const uint32_t X = dm_xpow8(GZ_SPAN);
    uint32_t acc = 0;
    for (uint32_t a = 0; a < tlen; a += GZ_SPAN) acc = dm_gfmul(acc, tlen - a >= GZ_SPAN ? X : dm_xpow8(tlen - a)) ^ cc[a / GZ_SPAN];
    return acc;
}
__global__ __launch_bounds__(256) void k_gz_translate(const uint16_t *sym, const GzWalkRow *rows, uint32_t nw, const uint8_t *wins, uint64_t T, uint8_t *out, uint64_t ntiles,
                                                      uint32_t *tilecrc, unsigned long long *bad)
{
    __shared__ uint32_t crctab[256];
    __shared__ uint32_t tile[256 * GZ_PITCH];
    __shared__ uint32_t cc[256];
    const uint64_t b = harc_bid();
    if (b >= ntiles) return;
    const uint32_t t = threadIdx.x;
    crctab[t] = im_crc_entry(t);
    const uint64_t t0 = b * GZ_TILE;
    const uint32_t tlen = T - t0 < GZ_TILE ? (uint32_t)(T - t0) : GZ_TILE;
    for (uint32_t q = t * 16; q < tlen; q += 4096) {
        const uint64_t p = t0 + q;
        const uint32_t m = tlen - q < 16 ? tlen - q : 16;
        uint32_t lo = 0, hi = nw;                                 // the walk that holds text byte p: the last whose text_off is <= p and that is not empty there
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (rows[mid].text_off <= p) lo = mid; else hi = mid; }
        uint32_t w = lo;
        uint64_t wend = rows[w].text_off + rows[w].text; uint32_t have = rows[w].have;
        uint32_t v[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            if (k >= m) break;
            while (p + k >= wend && w + 1 < nw) { w++; wend = rows[w].text_off + rows[w].text; have = rows[w].have; }
            uint8_t x = 0;
            const int rc = is_translate(sym[p + k], wins + (uint64_t)w * IS_WIN, have, &x);
            if (rc) atomicMin(bad, ((unsigned long long)w << 8) | (unsigned long long)rc);
            v[k >> 2] |= (uint32_t)x << (8 * (k & 3));
        }
        uint32_t *row = tile + (q / GZ_SPAN) * GZ_PITCH + (q % GZ_SPAN) / 4;
        row[0] = v[0]; row[1] = v[1]; row[2] = v[2]; row[3] = v[3];
        uint8_t *dst = out + p;
        if (m == 16 && ((uintptr_t)dst & 15u) == 0) *(uint4 *)dst = make_uint4(v[0], v[1], v[2], v[3]);
        else for (uint32_t k = 0; k < m; k++) dst[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    }
    __syncthreads();
    {   // span t
        const uint32_t a = t * GZ_SPAN, sl = a >= tlen ? 0 : tlen - a < GZ_SPAN ? tlen - a : GZ_SPAN;
        uint32_t c = 0xFFFFFFFFu;
        const uint32_t *row = tile + t * GZ_PITCH;
        for (uint32_t k = 0; k < sl; k++) c = crctab[(c ^ (row[k >> 2] >> (8 * (k & 3)))) & 0xFFu] ^ (c >> 8);
        cc[t] = sl ? c ^ 0xFFFFFFFFu : 0;
    }
    __syncthreads();
    if (tlen == GZ_TILE) {                                        // a full tile: a tree, x^(8 * 64 * s) squared from level to level
        uint32_t Xp = dm_xpow8(GZ_SPAN);
        for (uint32_t s = 1; s < 256; s <<= 1) {
            uint32_t v = 0;
            const bool mine = (t & (2 * s - 1)) == 0;
            if (mine) v = dm_gfmul(cc[t], Xp) ^ cc[t + s];
            __syncthreads();
            if (mine) cc[t] = v;
            __syncthreads();
            Xp = dm_gfmul(Xp, Xp);
        }
        if (t == 0) tilecrc[b] = cc[0];
    } else if (t == 0) tilecrc[b] = gz_fold_spans(cc, tlen);
}

static const char *gz_what(int rc)
{
    switch (rc) {
    case IM_E_TRUNC: return "the input ends inside a member";
    case IM_E_BTYPE: return "block type 3";
    case IM_E_STORED: return "stored block length does not match its complement";
    case IM_E_CODES: return "bad Huffman code lengths";
    case IM_E_SYMBOL: return "invalid Huffman code";
    case IM_E_DIST: return "distance before the start of the member";
    case IM_E_OVERFLOW: case IM_E_SHORT: return "a walk did not repeat its count";
    case IM_E_CRC: return "CRC-32 mismatch";
    case IM_E_GZHEADER: return "no gzip member header (magic 1f 8b, method 8, no reserved flag)";
    case IM_E_TRAILING: return "bytes behind the trailer that are no gzip member";
    case IM_E_LENGTH: return "the length of the text differs from ISIZE";
    default: return "corrupt stream";
    }
}

// ------------------------------------------------------------------------------------------------ the backend: where the bytes are and who walks them
struct GzBackend {
    uint64_t n = 0;                                               // compressed bytes at hand
    virtual ~GzBackend() {}
    virtual int peek(uint64_t off, uint64_t len, uint8_t *host) = 0;
    virtual int find(uint64_t base, uint64_t cb, uint64_t k0, uint64_t nk, std::vector<uint64_t> &cand) = 0;      // cand[i]: of chunk k0 + i
    virtual int count(const std::vector<GzRow> &rows, std::vector<IsWalk> &res, std::vector<int32_t> &rcs) = 0;
    // stages 4-6: the text of the walks -> bytes [text_off, text_off + T) of the output; win: the window in front of the first walk in, behind the last out;
    // *bad: ~0, or (walk << 8 | code)
    virtual int emit(const std::vector<GzWalkRow> &rows, uint64_t T, uint8_t *win, uint64_t text_off, std::vector<uint32_t> &tilecrc, unsigned long long *bad) = 0;
};

struct GzHost : GzBackend {
    const uint8_t *in = nullptr; uint8_t *out = nullptr;
    ImTables tab; uint32_t crctab[256];
    GzHost() { for (uint32_t i = 0; i < 256; i++) crctab[i] = im_crc_entry(i); }
    int peek(uint64_t off, uint64_t len, uint8_t *host) override { memcpy(host, in + off, (size_t)len); return HARC_AMD_OK; }
    int find(uint64_t base, uint64_t cb, uint64_t k0, uint64_t nk, std::vector<uint64_t> &cand) override
    {
        cand.assign((size_t)nk, IS_NONE);
        for (uint64_t i = 0; i < nk; i++) {
            uint64_t hi = base + (k0 + i + 1) * cb; if (hi > n) hi = n;
            cand[(size_t)i] = is_find(in, n, (base + (k0 + i) * cb) * 8, hi * 8, tab);
        }
        return HARC_AMD_OK;
    }
    int count(const std::vector<GzRow> &rows, std::vector<IsWalk> &res, std::vector<int32_t> &rcs) override
    {
        res.resize(rows.size()); rcs.resize(rows.size());
        for (size_t i = 0; i < rows.size(); i++) {
            IsWalk w; w.end_bit = rows[i].bit; w.text = 0; w.final = 0; w.more = 0;
            rcs[i] = rows[i].bit == IS_NONE ? -1 : is_count(in, n, rows[i].bit, rows[i].stop_bit, tab, &w);
            res[i] = w;
        }
        return HARC_AMD_OK;
    }
    int emit(const std::vector<GzWalkRow> &rows, uint64_t T, uint8_t *win, uint64_t text_off, std::vector<uint32_t> &tilecrc, unsigned long long *bad) override
    {
        *bad = ~0ull;
        std::vector<uint16_t> sym((size_t)T + 1);
        std::vector<uint8_t> wins((rows.size() + 1) * (size_t)IS_WIN);
        memcpy(wins.data(), win, IS_WIN);
        for (size_t i = 0; i < rows.size(); i++) {
            const GzWalkRow &r = rows[i];
            IsWalk w;
            int rc = is_walk(in, n, r.bit, r.end_bit, tab, sym.data() + r.text_off, r.text, &w);
            if (!rc && (w.end_bit != r.end_bit || w.text != r.text)) rc = IM_E_SHORT;
            if (rc) { *bad = ((unsigned long long)i << 8) | (unsigned long long)rc; return HARC_AMD_OK; }
        }
        for (size_t i = 0; i < rows.size(); i++)
            for (uint32_t j = 0; j < IS_WIN; j++) wins[(i + 1) * IS_WIN + j] = is_window_byte(wins.data() + i * IS_WIN, sym.data() + rows[i].text_off, rows[i].text, j);
        uint8_t *dst = out + text_off;
        for (size_t i = 0; i < rows.size(); i++)
            for (uint64_t k = 0; k < rows[i].text; k++) {
                const int rc = is_translate(sym[(size_t)(rows[i].text_off + k)], wins.data() + i * IS_WIN, rows[i].have, dst + rows[i].text_off + k);
                if (rc) { *bad = ((unsigned long long)i << 8) | (unsigned long long)rc; return HARC_AMD_OK; }
            }
        tilecrc.clear();
        uint32_t cc[GZ_TILE / GZ_SPAN];
        for (uint64_t t0 = 0; t0 < T; t0 += GZ_TILE) {
            const uint32_t tlen = T - t0 < GZ_TILE ? (uint32_t)(T - t0) : GZ_TILE;
            for (uint32_t a = 0; a < tlen; a += GZ_SPAN) cc[a / GZ_SPAN] = dm_crc_bytes(dst + t0 + a, tlen - a < GZ_SPAN ? tlen - a : GZ_SPAN, crctab);
            tilecrc.push_back(gz_fold_spans(cc, tlen));
        }
        memcpy(win, wins.data() + rows.size() * IS_WIN, IS_WIN);
        return HARC_AMD_OK;
    }
};

struct GzDevice : GzBackend {
    harc_amd_ctx *c = nullptr; const uint8_t *d_in = nullptr;
    uint8_t *d_out = nullptr;                                     // the whole output (device call), or ...
    DevBuf *stage = nullptr; FileDrain *drain = nullptr;          // ... a buffer of the call's that every turn's text goes through on its way to the file
    LapTimer *lap = nullptr;
    int peek(uint64_t off, uint64_t len, uint8_t *host) override
    {
        HIP_TRY(hipMemcpyAsync(host, d_in + off, (size_t)len, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return HARC_AMD_OK;
    }
    int find(uint64_t base, uint64_t cb, uint64_t k0, uint64_t nk, std::vector<uint64_t> &cand) override
    {
        cand.assign((size_t)nk, IS_NONE);
        if (!nk) return HARC_AMD_OK;
        PoolScope scope(c);
        const uint32_t waves = nk < GZ_WAVES ? (uint32_t)nk : GZ_WAVES;
        ImTables *tabs = nullptr; RC_TRY(dalloc(c, &tabs, (size_t)waves * 64));
        unsigned long long *d_cand = nullptr; RC_TRY(dalloc(c, &d_cand, (size_t)nk));
        hipLaunchKernelGGL(k_gz_find, dim3(waves), dim3(64), 0, c->stream, d_in, n, base, cb, k0, nk, tabs, d_cand);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cand.data(), d_cand, (size_t)nk * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (lap) lap->lap("finder");
        return HARC_AMD_OK;
    }
    int count(const std::vector<GzRow> &rows, std::vector<IsWalk> &res, std::vector<int32_t> &rcs) override
    {
        const uint32_t nr = (uint32_t)rows.size();
        res.resize(nr); rcs.resize(nr);
        if (!nr) return HARC_AMD_OK;
        PoolScope scope(c);
        const uint32_t nslots = ((nr < GZ_SLOTS ? nr : GZ_SLOTS) + 63u) & ~63u;
        GzRow *d_rows = nullptr; RC_TRY(dalloc(c, &d_rows, (size_t)nr));
        IsWalk *d_res = nullptr; RC_TRY(dalloc(c, &d_res, (size_t)nr));
        int32_t *d_rcs = nullptr; RC_TRY(dalloc(c, &d_rcs, (size_t)nr));
        ImTables *tabs = nullptr; RC_TRY(dalloc(c, &tabs, (size_t)nslots));
        HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), (size_t)nr * sizeof(GzRow), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_gz_count, dim3(nslots / 64), dim3(64), 0, c->stream, d_in, n, (const GzRow *)d_rows, nr, tabs, nslots, d_res, d_rcs);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(res.data(), d_res, (size_t)nr * sizeof(IsWalk), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rcs.data(), d_rcs, (size_t)nr * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (lap && nr > 1) lap->lap("count");
        return HARC_AMD_OK;
    }
    int emit(const std::vector<GzWalkRow> &rows, uint64_t T, uint8_t *win, uint64_t text_off, std::vector<uint32_t> &tilecrc, unsigned long long *bad) override
    {
        *bad = ~0ull;
        const uint32_t nw = (uint32_t)rows.size();
        uint8_t *dst = d_out ? d_out + text_off : nullptr;
        if (stage) { RC_TRY(dev_reserve(stage, (size_t)T)); dst = (uint8_t *)stage->p; }
        PoolScope scope(c);
        const uint64_t ntiles = (T + GZ_TILE - 1) / GZ_TILE;
        const uint32_t nslots = ((nw < GZ_SLOTS ? nw : GZ_SLOTS) + 63u) & ~63u;
        GzWalkRow *d_rows = nullptr; RC_TRY(dalloc(c, &d_rows, (size_t)nw));
        uint16_t *d_sym = nullptr; RC_TRY(dalloc(c, &d_sym, (size_t)T));
        uint8_t *d_wins = nullptr; RC_TRY(dalloc(c, &d_wins, ((size_t)nw + 1) * IS_WIN));
        ImTables *tabs = nullptr; RC_TRY(dalloc(c, &tabs, (size_t)nslots));
        uint32_t *d_crc = nullptr; RC_TRY(dalloc(c, &d_crc, (size_t)ntiles));
        unsigned long long *d_bad = nullptr; RC_TRY(dalloc(c, &d_bad, 1));
        HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), (size_t)nw * sizeof(GzWalkRow), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_wins, win, IS_WIN, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
        hipLaunchKernelGGL(k_gz_write, dim3(nslots / 64), dim3(64), 0, c->stream, d_in, n, (const GzWalkRow *)d_rows, nw, d_sym, tabs, nslots, d_bad);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (lap) lap->lap("write");
        if (*bad != ~0ull) return HARC_AMD_OK;                     // the symbols are not all there: nothing reads them
        hipLaunchKernelGGL(k_gz_window, dim3(1), dim3(1024), 0, c->stream, (const uint16_t *)d_sym, (const GzWalkRow *)d_rows, nw, d_wins);
        HIP_TRY(hipGetLastError());
        if (lap) { HIP_TRY(hipStreamSynchronize(c->stream)); lap->lap("window"); }
        hipLaunchKernelGGL(k_gz_translate, harc_fold256(ntiles), dim3(256), 0, c->stream, (const uint16_t *)d_sym, (const GzWalkRow *)d_rows, nw, (const uint8_t *)d_wins, T, dst, ntiles,
                           d_crc, d_bad);
        HIP_TRY(hipGetLastError());
        tilecrc.resize((size_t)ntiles);
        HIP_TRY(hipMemcpyAsync(tilecrc.data(), d_crc, (size_t)ntiles * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(win, d_wins + (size_t)nw * IS_WIN, IS_WIN, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (lap) lap->lap("translate");
        if (drain && *bad == ~0ull) RC_TRY(drain->put(dst, (size_t)T, text_off));
        return HARC_AMD_OK;
    }
};

// ------------------------------------------------------------------------------------------------ plan and execution, once for every backend
struct GzSeg {                                                    // what one turn of stages 4-6 produces: walks of one member
    std::vector<GzWalkRow> rows; uint64_t T = 0;
    bool starts_member = false, ends_member = false;
    uint32_t crc = 0, isize = 0; uint64_t trailer = 0;            // ends_member: the trailer's numbers and its byte in the input at hand
};
struct GzState {
    // the plan's: between members (pos) or inside one (the bit of the next block)
    bool in_member = false, fresh = false; uint64_t members_seen = 0;
    uint64_t bit = 0;
    // the execution's: the member so far
    uint8_t win[IS_WIN]; uint32_t have = 0, crc = 0; uint64_t len = 0;
    uint64_t text_off = 0;
};
static int gz_refuse(uint64_t file_byte, int rc)
{
    harc_set_error("gunzip: compressed byte %llu: %s", (unsigned long long)file_byte, gz_what(rc));
    return HARC_AMD_EINVAL;
}
static uint64_t gz_chunk_bytes(uint64_t chunk_bytes)
{
    uint64_t cb = chunk_bytes ? chunk_bytes : env_u64("HARC_AMD_GUNZIP_CHUNK", GZ_CHUNK);
    return cb < 64 ? 64 : cb;
}

// The input at hand, B.n bytes whose first is byte file_off of the file, from the state on: headers, stages 1-3, trailers -> the turns to execute, and how many
// bytes are done with (*consumed; the rest is carried in front of the next piece, the state's bit offset counts from there).  last: nothing follows.
static int gz_plan(GzBackend &B, bool last, uint64_t cb, uint64_t budget, uint64_t file_off, GzState &S, harc_amd_gunzip_stats *st, std::vector<GzSeg> &segs, uint64_t *consumed)
{
    const uint64_t n = B.n;
    uint64_t pos = 0, e = S.bit, base = S.bit >> 3;
    std::vector<uint8_t> hb;
    std::vector<uint64_t> cand; std::vector<GzRow> rows; std::vector<IsWalk> res; std::vector<int32_t> rcs;
    for (;;) {
        bool starts = false;
        if (!S.in_member) {
            if (pos == n) {
                if (!last) { *consumed = pos; S.bit = 0; return HARC_AMD_OK; }
                if (!S.members_seen) return gz_refuse(file_off + pos, IM_E_GZHEADER);
                *consumed = pos; return HARC_AMD_OK;
            }
            const uint64_t avail = n - pos < GZ_HDR_PEEK ? n - pos : GZ_HDR_PEEK;
            hb.resize((size_t)avail);
            RC_TRY(B.peek(pos, avail, hb.data()));
            uint64_t hdr = 0;
            const int rc = gz_header(hb.data(), avail, &hdr);
            if (rc == IM_E_TRUNC) {
                if (!last && avail < GZ_HDR_PEEK) { *consumed = pos; S.bit = 0; return HARC_AMD_OK; }
                return gz_refuse(file_off + (last && avail < GZ_HDR_PEEK ? n : pos), avail < GZ_HDR_PEEK ? IM_E_TRUNC : IM_E_GZHEADER);
            }
            if (rc) return gz_refuse(file_off + pos, S.members_seen ? IM_E_TRAILING : IM_E_GZHEADER);
            S.in_member = true; starts = true;
            base = pos; e = (pos + hdr) * 8;
        }
        // stages 1 and 2: chunks of cb bytes from `base`; the chunk that holds e starts at e, every later one at what the finder gives it
        std::vector<GzWalkRow> walks;
        enum { MORE, CUT, FINAL } ended = MORE;
        if ((e >> 3) < n) {
            const uint64_t nk = (n - base + cb - 1) / cb, k0 = ((e >> 3) - base) / cb;
            auto chunk_end = [&](uint64_t k) { const uint64_t h = base + (k + 1) * cb; return (h < n ? h : n) * 8; };
            RC_TRY(B.find(base, cb, k0 + 1, nk - k0 - 1, cand));
            rows.clear();
            rows.push_back(GzRow{ e, chunk_end(k0) });
            uint64_t found = 0, used = 0;
            for (uint64_t k = k0 + 1; k < nk; k++) { rows.push_back(GzRow{ cand[(size_t)(k - k0 - 1)], chunk_end(k) }); found += cand[(size_t)(k - k0 - 1)] != IS_NONE; }
            RC_TRY(B.count(rows, res, rcs));
            st->chunks += nk - k0; st->starts_found += found;
            // stage 3, the chain
            uint64_t total = 0;
            std::vector<GzRow> one(1); std::vector<IsWalk> r1; std::vector<int32_t> rc1;
            while ((e >> 3) < n) {
                const uint64_t k = ((e >> 3) - base) / cb;
                IsWalk w; int rc;
                if (rows[(size_t)(k - k0)].bit == e && rcs[(size_t)(k - k0)] == 0) { w = res[(size_t)(k - k0)]; rc = 0; used += k > k0; }
                else {
                    one[0] = GzRow{ e, chunk_end(k) };
                    RC_TRY(B.count(one, r1, rc1));
                    w = r1[0]; rc = rc1[0]; st->repair_walks++;
                }
                if (rc) return gz_refuse(file_off + (w.end_bit >> 3), rc);
                if (w.end_bit == e) break;                        // not one whole block from here: bytes behind the end are needed
                if (total + w.text > budget) {
                    if (walks.empty()) { harc_set_error("gunzip: one walk from compressed byte %llu gives %llu bytes of text, more than the %llu of HARC_AMD_GUNZIP_BUDGET", (unsigned long long)(file_off + (e >> 3)), (unsigned long long)w.text, (unsigned long long)budget); return HARC_AMD_ENOMEM; }
                    ended = CUT; break;
                }
                GzWalkRow wr; wr.bit = e; wr.end_bit = w.end_bit; wr.text_off = total; wr.text = w.text; wr.have = 0; wr.pad = 0;
                walks.push_back(wr);
                total += w.text; e = w.end_bit;
                if (w.final) { ended = FINAL; break; }
                if (w.more) break;
            }
            st->starts_dropped += found - used;
        }
        GzSeg seg; seg.starts_member = starts || S.fresh; S.fresh = false;
        if (ended == FINAL) {
            const uint64_t tb = (e + 7) >> 3;
            if (tb + 8 > n) {
                if (last) return gz_refuse(file_off + n, IM_E_TRUNC);
                e = walks.back().bit; walks.pop_back(); ended = MORE;     // the trailer comes with the next piece: so does the walk in front of it
            } else {
                uint8_t tr[8];
                RC_TRY(B.peek(tb, 8, tr));
                seg.ends_member = true; seg.crc = im_le32(tr); seg.isize = im_le32(tr + 4); seg.trailer = tb;
            }
        }
        if (!walks.empty()) {
            seg.rows.swap(walks);
            seg.T = seg.rows.back().text_off + seg.rows.back().text;
            segs.push_back(std::move(seg));
        } else if (seg.starts_member) S.fresh = true;             // the member's first turn is still to come
        if (ended == FINAL) {
            st->members++; S.members_seen++; S.in_member = false;
            pos = segs.back().trailer + 8;
            continue;
        }
        if (ended == CUT) { base = e >> 3; continue; }
        if (last) return gz_refuse(file_off + n, IM_E_TRUNC);
        *consumed = e >> 3; S.bit = e & 7u;
        return HARC_AMD_OK;
    }
}
// stages 4-6 of every turn, then the member's CRC-32 and length against its trailer
static int gz_exec(GzBackend &B, uint64_t file_off, GzState &S, std::vector<GzSeg> &segs, harc_amd_gunzip_stats *st)
{
    const uint32_t XT = dm_xpow8(GZ_TILE);
    std::vector<uint32_t> tilecrc;
    for (GzSeg &g : segs) {
        if (g.starts_member) { memset(S.win, 0, IS_WIN); S.have = 0; S.crc = 0; S.len = 0; }
        if (g.T) {
            uint32_t have = S.have;
            for (GzWalkRow &r : g.rows) { r.have = have; have = is_window_have(have, r.text); }
            unsigned long long bad = ~0ull;
            RC_TRY(B.emit(g.rows, g.T, S.win, S.text_off, tilecrc, &bad));
            if (bad != ~0ull) return gz_refuse(file_off + (g.rows[(size_t)(bad >> 8)].bit >> 3), (int)(bad & 255));
            for (size_t i = 0; i < tilecrc.size(); i++) {
                const uint64_t l = g.T - (uint64_t)i * GZ_TILE;
                S.crc = dm_gfmul(S.crc, l >= GZ_TILE ? XT : dm_xpow8((uint32_t)l)) ^ tilecrc[i];
            }
            S.have = have; S.len += g.T; S.text_off += g.T; st->text_bytes += g.T;
        }
        if (g.ends_member) {
            if (S.crc != g.crc) return gz_refuse(file_off + g.trailer, IM_E_CRC);
            if ((uint32_t)S.len != g.isize) return gz_refuse(file_off + g.trailer + 4, IM_E_LENGTH);
        }
    }
    return HARC_AMD_OK;
}
static uint64_t gz_text_of(const std::vector<GzSeg> &segs) { uint64_t t = 0; for (const GzSeg &g : segs) t += g.T; return t; }

// a whole input in one piece
static int gz_whole(GzBackend &B, const char *who, uint64_t chunk_bytes, bool write, uint64_t out_capacity, uint64_t *n_out, harc_amd_gunzip_stats *stats)
{
    harc_amd_gunzip_stats st; memset(&st, 0, sizeof st);
    std::vector<GzSeg> segs; uint64_t consumed = 0;
    GzState *S = new GzState; std::unique_ptr<GzState> own(S);
    RC_TRY(gz_plan(B, true, gz_chunk_bytes(chunk_bytes), env_u64("HARC_AMD_GUNZIP_BUDGET", (uint64_t)1 << 30), 0, *S, &st, segs, &consumed));
    const uint64_t T = gz_text_of(segs);
    *n_out = T;
    if (write) {
        if (out_capacity < T) { harc_set_error("%s: the text is %llu bytes, the buffer %llu", who, (unsigned long long)T, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
        RC_TRY(gz_exec(B, 0, *S, segs, &st));
    } else st.text_bytes = T;
    if (stats) *stats = st;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_gunzip_host(const uint8_t *gz, uint64_t n_bytes, uint64_t chunk_bytes, char *out, uint64_t out_capacity, uint64_t *n_out, harc_amd_gunzip_stats *stats)
{
    if ((n_bytes && !gz) || !n_out) { harc_set_error("gunzip_host: bad arguments"); return HARC_AMD_EINVAL; }
    GzHost *B = new GzHost; std::unique_ptr<GzHost> own(B);
    B->n = n_bytes; B->in = gz; B->out = (uint8_t *)out;
    return gz_whole(*B, "gunzip_host", chunk_bytes, out != nullptr, out_capacity, n_out, stats);
}

extern "C" int harc_amd_gunzip_device(harc_amd_ctx *c, const uint8_t *d_gz, uint64_t n_bytes, uint64_t chunk_bytes, char *d_out, uint64_t out_capacity, uint64_t *n_out,
                                      harc_amd_gunzip_stats *stats)
{
    if (!c || (n_bytes && !d_gz) || !n_out) { harc_set_error("gunzip_device: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    GzDevice B; B.n = n_bytes; B.c = c; B.d_in = d_gz; B.d_out = (uint8_t *)d_out;
    LapTimer lap{ "[gunzip]" };
    if (lap.on) B.lap = &lap;
    return gz_whole(B, "gunzip_device", chunk_bytes, d_out != nullptr, out_capacity, n_out, stats);
}

extern "C" int harc_amd_gunzip_files(const harc_amd_params *params, const char *gz_path, const char *out_path, harc_amd_gunzip_stats *stats)
{
    if (!params || !gz_path || !out_path) { harc_set_error("gunzip_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t gsz = 0;
    if (!file_size(gz_path, &gsz)) { harc_set_error("cannot open %s", gz_path); return HARC_AMD_EIO; }
    {   // the same file under two names must not be opened for writing: the refusal comes before the guard that removes the output
        struct stat a, b;
        if (!strcmp(gz_path, out_path) || (stat(gz_path, &a) == 0 && stat(out_path, &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)) {
            harc_set_error("gunzip_files: the output %s is the input", out_path); return HARC_AMD_EINVAL; }
    }
    if (gsz < 18) { harc_set_error("gunzip: %s holds %llu bytes: no gzip member is that short", gz_path, (unsigned long long)gsz); return HARC_AMD_EINVAL; }
    OutFileGuard outguard{ out_path };
    const uint64_t piece = env_u64("HARC_AMD_GUNZIP_PIECE", (uint64_t)64 << 20), budget = env_u64("HARC_AMD_GUNZIP_BUDGET", (uint64_t)1 << 30), cb = gz_chunk_bytes(0);
    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom g[2];                                                // the feeder's and the drain's
    RC_TRY(ring_split(c, 2, 8, "gunzip", g, gsz <= ((uint64_t)16 << 20) ? (size_t)4 << 20 : 0));     // a small file does not pin a ring of 1 GiB
    harc_amd_gunzip_stats st; memset(&st, 0, sizeof st);
    GzState *S = new GzState; std::unique_ptr<GzState> own(S);
    DevBuf stage{ c };
    LapTimer lap{ "[gunzip]" };
    double t_read = 0;
    {
        // DEFLATE gives at most 1032 bytes of text per compressed byte: the file is mapped that long, its blocks are allocated as the text arrives, and it is cut at the end
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)(gsz * 1032 + 4096), &g[1], true));
        const Pieces pieces = byte_pieces(0, gsz, piece);
        FileFeeder feed(c, gz_path);
        RC_TRY(feed.start(pieces, g[0]));
        CarriedText in(c);
        GzDevice B; B.c = c; B.stage = &stage; B.drain = &drain;
        if (lap.on) B.lap = &lap;
        std::vector<GzSeg> segs;
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t len = pieces[p].second - pieces[p].first, file_off = pieces[p].first - in.carry;
            RC_TRY(in.take(feed, p, len, &t_read));
            HIP_TRY(hipStreamSynchronize(c->stream));
            lap.lap("upload");
            B.d_in = (const uint8_t *)in.text(); B.n = in.carry + len;
            const bool last = p + 1 == pieces.size();
            // the piece is planned whole, then its text is produced turn by turn, each through the same buffers
            uint64_t consumed = 0;
            segs.clear();
            RC_TRY(gz_plan(B, last, cb, budget, file_off, *S, &st, segs, &consumed));
            RC_TRY(gz_exec(B, file_off, *S, segs, &st));
            if (!last) RC_TRY(in.carry_from(consumed, B.n - consumed));
        }
        drain.set_final_size(S->text_off);
        RC_TRY(drain.finish());
        lap.lap("file written");
    }
    if (stats) *stats = st;
    outguard.ok = true;
    return HARC_AMD_OK;
}
