// recover.hip -- the recovery record behind ./harc -c -P and -R (README: "-P and what it promises", "The recovery record (X.hr)").  The arithmetic, the geometry and
// the head of the record are gf_block.h's; this file gives them their lanes and holds the calls of the C-ABI.
//   k_block_digests  the digest of every block of a span resident in device memory, one launch: a workgroup per block, aligned 16-byte loads, sixteen terms a lane
//                    and iteration, a reduction across the wave and then across the workgroup's four waves; no atomic.
//   k_gf_combine     out[q] = XOR_s coef[q][s] * src[s] over B bytes, for a batch of jobs (blockIdx.z: the groups of a span).  A lane owns 16 bytes of the block and
//                    walks the sources; the eight doublings of a source word are made once, on packed words, and each of the eight outputs a pass keeps in registers
//                    XORs in those its coefficient names.  The coefficients of a source arrive as one 8-byte word, the same for every lane.
// One driver makes, checks and repairs; it is written against RcBackend, which the device (DevBackend: pinned ring, kernels) and the host twin (HostBackend: pread,
// gf_block.h's functions) implement.
#include "devutil.h"
#include "check_block.h"
#include "gf_block.h"
#include "fileio.h"
#include <stdarg.h>

#define GF_T 256
#define GF_TILE 8
#define GF_BATCH 1024             // jobs of one launch

struct GfJob { uint32_t src0, out0, coef0, ns, e; };              // first source pointer, first output pointer, first coefficient word of the job; sources, outputs

__global__ __launch_bounds__(GF_T) void k_block_digests(const uint8_t *base, uint64_t nblocks, uint32_t B, uint32_t last_len, unsigned long long *out)
{
    __shared__ uint64_t part[GF_T / 64];
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {  // (the same trips for every lane of the workgroup)
        const uint32_t len = b + 1 == nblocks ? last_len : B;
        const uint4 *p = (const uint4 *)(base + b * (uint64_t)B);
        const uint32_t nch = (len + 15) >> 4;
        uint64_t d = 0; uint32_t nl = 0;
        for (uint32_t k = threadIdx.x; k < nch; k += GF_T) {
            const uint4 v = p[k];
            const uint32_t a = k << 4;
            uint32_t keep = 0xFFFFu;
            if (a + 16 > len) keep >>= a + 16 - len;              // (the last chunk of a short block alone)
            ck_word((uint64_t)v.x | ((uint64_t)v.y << 32), keep & 0xFFu, a, &d, &nl);
            ck_word((uint64_t)v.z | ((uint64_t)v.w << 32), keep >> 8, (uint64_t)a + 8, &d, &nl);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += shfl_u64_any(d, o);
        if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = d;
        __syncthreads();
        if (threadIdx.x == 0) { uint64_t s = 0; for (int w = 0; w < GF_T / 64; w++) s += part[w]; out[b] = s; }
        __syncthreads();
    }
}

__device__ __forceinline__ uint4 gf_x2_u4(uint4 w) { return make_uint4(gf_x2_word(w.x), gf_x2_word(w.y), gf_x2_word(w.z), gf_x2_word(w.w)); }

// chunks: 16-byte chunks of a block.  ptrs: the jobs' source and output blocks.  coef: per job, pass and source one word of GF_TILE coefficients (byte q: output
// pass * GF_TILE + q; 0 behind the job's last output)
__global__ __launch_bounds__(GF_T) void k_gf_combine(const GfJob *jobs, const uint4 *const *ptrs, const uint2 *coef, uint32_t chunks)
{
    const GfJob jb = jobs[blockIdx.z];
    const uint32_t q0 = blockIdx.y * GF_TILE;
    if (q0 >= jb.e) return;                                       // (the whole workgroup)
    const uint32_t lane = blockIdx.x * GF_T + threadIdx.x;
    if (lane >= chunks) return;
    const uint4 *const *src = ptrs + jb.src0;
    const uint2 *ct = coef + jb.coef0 + (size_t)blockIdx.y * jb.ns;
    uint4 acc[GF_TILE];
#pragma unroll
    for (int q = 0; q < GF_TILE; q++) acc[q] = make_uint4(0, 0, 0, 0);
    uint4 v = src[0][lane];
    for (uint32_t s = 0; s < jb.ns; s++) {
        const uint4 nxt = src[s + 1 < jb.ns ? s + 1 : s][lane];   // the next source is on its way while this one is worked
        const uint2 c = ct[s];
        uint4 w = v;
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
#pragma unroll
            for (int q = 0; q < GF_TILE; q++) {
                const uint32_t cw = q < 4 ? c.x : c.y;
                if ((cw >> (8 * (q & 3) + bit)) & 1u) { acc[q].x ^= w.x; acc[q].y ^= w.y; acc[q].z ^= w.z; acc[q].w ^= w.w; }      // the same way for every lane
            }
            if (bit < 7) w = gf_x2_u4(w);
        }
        v = nxt;
    }
    uint4 *const *out = (uint4 *const *)(ptrs + jb.out0);
#pragma unroll
    for (int q = 0; q < GF_TILE; q++) if (q0 + q < jb.e) out[q0 + q][lane] = acc[q];
}

// ------------------------------------------------------------------------------------------------ the two launches
struct RcJob { std::vector<uint64_t> src, out; std::vector<uint8_t> coef; };      // blocks by address (device) or offset (host backend); coef: out.size() x src.size()

static int rc_digests_launch(harc_amd_ctx *c, const void *d_data, uint64_t nblocks, uint32_t B, uint32_t last_len, uint64_t *out)
{
    if (!nblocks) return HARC_AMD_OK;
    PoolScope scope(c);
    unsigned long long *d_out = nullptr;
    RC_TRY(dalloc(c, &d_out, (size_t)nblocks));
    const unsigned grid = (unsigned)(nblocks < (1u << 20) ? nblocks : (1u << 20));
    hipLaunchKernelGGL(k_block_digests, dim3(grid), dim3(GF_T), 0, c->stream, (const uint8_t *)d_data, nblocks, B, last_len, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)nblocks * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HARC_AMD_OK;
}
// the jobs on the stream, GF_BATCH a launch; nothing is waited for.  Every address is a multiple of 16 and names B bytes (the callers hold to that)
static int rc_combine_launch(harc_amd_ctx *c, uint32_t B, const std::vector<RcJob> &jobs, KernelTimer *timer = nullptr)
{
    const uint32_t chunks = B / 16;
    for (size_t j0 = 0; j0 < jobs.size(); j0 += GF_BATCH) {
        const size_t j1 = jobs.size() - j0 < GF_BATCH ? jobs.size() : j0 + GF_BATCH;
        std::vector<GfJob> hj; std::vector<uint64_t> hp; std::vector<uint64_t> hc;
        uint32_t passes = 0;
        for (size_t j = j0; j < j1; j++) {
            const RcJob &J = jobs[j];
            const uint32_t ns = (uint32_t)J.src.size(), e = (uint32_t)J.out.size(), np = (e + GF_TILE - 1) / GF_TILE;
            GfJob g{ (uint32_t)hp.size(), (uint32_t)(hp.size() + ns), (uint32_t)hc.size(), ns, e };
            hp.insert(hp.end(), J.src.begin(), J.src.end()); hp.insert(hp.end(), J.out.begin(), J.out.end());
            for (uint32_t p = 0; p < np; p++)
                for (uint32_t s = 0; s < ns; s++) {
                    uint64_t w = 0;
                    for (uint32_t q = 0; q < GF_TILE && p * GF_TILE + q < e; q++) w |= (uint64_t)J.coef[(size_t)(p * GF_TILE + q) * ns + s] << (8 * q);
                    hc.push_back(w);
                }
            if (np > passes) passes = np;
            hj.push_back(g);
        }
        PoolScope scope(c);                                       // (what the next launch puts in the same place is copied behind this kernel, on the same stream)
        GfJob *d_jobs = nullptr; uint64_t *d_ptrs = nullptr, *d_coef = nullptr;
        RC_TRY(dalloc(c, &d_jobs, hj.size())); RC_TRY(dalloc(c, &d_ptrs, hp.size())); RC_TRY(dalloc(c, &d_coef, hc.size()));
        HIP_TRY(hipMemcpyAsync(d_jobs, hj.data(), hj.size() * sizeof(GfJob), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_ptrs, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_coef, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                 // the three host vectors go at the end of this trip
        if (timer) RC_TRY(timer->begin(c->stream));                 // (a timed call is one launch)
        hipLaunchKernelGGL(k_gf_combine, dim3((chunks + GF_T - 1) / GF_T, passes, (unsigned)hj.size()), dim3(GF_T), 0, c->stream, (const GfJob *)d_jobs,
                           (const uint4 *const *)d_ptrs, (const uint2 *)d_coef, chunks);
        HIP_TRY(hipGetLastError());
        if (timer) RC_TRY(timer->end_mark(c->stream));
    }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_block_digests_device(harc_amd_ctx *c, const void *d_data, uint64_t n_blocks, uint32_t block_bytes, uint32_t last_bytes, uint64_t *out)
{
    if (!c || !out || (n_blocks && !d_data)) { harc_set_error("block_digests_device: bad arguments"); return HARC_AMD_EINVAL; }
    if (block_bytes < 16 || block_bytes > GF_MAX_B || block_bytes % 16 || ((uintptr_t)d_data & 15u) || last_bytes < 1 || last_bytes > block_bytes) {
        harc_set_error("block_digests_device: blocks of %u bytes, the last of %u, at %p: a block is a multiple of 16 bytes from 16 to 2^24, the last holds 1 .. block bytes, the data is 16-byte aligned",
                       block_bytes, last_bytes, d_data);
        return HARC_AMD_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->P.device));
    return rc_digests_launch(c, d_data, n_blocks, block_bytes, last_bytes, out);
}
extern "C" int harc_amd_block_digests_host(const void *data, uint64_t n_blocks, uint32_t block_bytes, uint32_t last_bytes, uint64_t *out)
{
    if (!out || (n_blocks && !data) || block_bytes < 1 || last_bytes < 1 || last_bytes > block_bytes) { harc_set_error("block_digests_host: bad arguments"); return HARC_AMD_EINVAL; }
    for (uint64_t b = 0; b < n_blocks; b++) out[b] = gf_block_digest_host((const uint8_t *)data + b * block_bytes, b + 1 == n_blocks ? last_bytes : block_bytes);
    return HARC_AMD_OK;
}
static int rc_combine_args(const char *who, uint32_t B, int32_t ns, const void *const *src, int32_t e, void *const *out, const uint8_t *coef, bool aligned)
{
    if (!src || !out || !coef || ns < 1 || ns > 256 || e < 1 || e > 128 || B < 16 || B > GF_MAX_B || B % 16) {
        harc_set_error("%s: %d sources (1 .. 256), %d outputs (1 .. 128), blocks of %u bytes (a multiple of 16 from 16 to 2^24)", who, ns, e, B); return HARC_AMD_EINVAL; }
    for (int k = 0; k < ns + e; k++) {
        const void *p = k < ns ? src[k] : out[k - ns];
        if (!p || (aligned && ((uintptr_t)p & 15u))) { harc_set_error("%s: block %d is null or not 16-byte aligned", who, k); return HARC_AMD_EINVAL; }
    }
    return HARC_AMD_OK;
}
extern "C" int harc_amd_gf_combine_device(harc_amd_ctx *c, uint32_t block_bytes, int32_t ns, const void *const *d_src, int32_t e, void *const *d_out, const uint8_t *coef)
{
    if (!c) { harc_set_error("gf_combine_device: bad arguments"); return HARC_AMD_EINVAL; }
    RC_TRY(rc_combine_args("gf_combine_device", block_bytes, ns, d_src, e, d_out, coef, true));
    HIP_TRY(hipSetDevice(c->P.device));
    std::vector<RcJob> jobs(1);
    for (int s = 0; s < ns; s++) jobs[0].src.push_back((uint64_t)(uintptr_t)d_src[s]);
    for (int q = 0; q < e; q++) jobs[0].out.push_back((uint64_t)(uintptr_t)d_out[q]);
    jobs[0].coef.assign(coef, coef + (size_t)e * ns);
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(rc_combine_launch(c, block_bytes, jobs, &timer));
    RC_TRY(timer.end_wait());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (trace) fprintf(stderr, "[recovery] device call: %d sources, %d outputs of %u bytes, kernel %.3f ms (%.1f GB/s of source bytes)\n", ns, e, block_bytes, 1e3 * seconds,
                       seconds > 0 ? 1e-9 * (double)ns * block_bytes / seconds : 0.0);
    return HARC_AMD_OK;
}
// one job in host memory, on packed words
static void rc_combine_host(uint32_t B, const uint8_t *const *src, int ns, uint8_t *const *out, int e, const uint8_t *coef)
{
    for (int q = 0; q < e; q++)
        for (uint32_t a = 0; a < B; a += 4) {
            uint32_t r = 0, w;
            for (int s = 0; s < ns; s++) { memcpy(&w, src[s] + a, 4); r ^= gf_mul_word(w, coef[(size_t)q * ns + s]); }
            memcpy(out[q] + a, &r, 4);
        }
}
extern "C" int harc_amd_gf_combine_host(uint32_t block_bytes, int32_t ns, const void *const *src, int32_t e, void *const *out, const uint8_t *coef)
{
    RC_TRY(rc_combine_args("gf_combine_host", block_bytes, ns, src, e, out, coef, false));
    rc_combine_host(block_bytes, (const uint8_t *const *)src, ns, (uint8_t *const *)out, e, coef);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ who holds the bytes and computes
// Two resident areas: A (what is read: a span of a file, the blocks of a group) and O (what is made).  Offsets are bytes, multiples of 16.
struct RcBackend {
    virtual ~RcBackend() {}
    virtual int reserve(size_t a_bytes, size_t o_bytes) = 0;
    virtual int open(const std::string &path, const std::vector<std::pair<uint64_t, uint64_t>> &pieces) = 0;     // byte ranges of one file, in file order
    virtual int piece(size_t p, size_t a_at) = 0;                 // ... piece p -> A[a_at ..)
    virtual void close() = 0;
    virtual int upload(size_t a_at, const uint8_t *h, size_t n) = 0;
    virtual int zero(size_t a_at, size_t n) = 0;
    virtual int digests(bool o, size_t at, uint64_t nblocks, uint32_t B, uint32_t last_len, uint64_t *out) = 0;
    virtual int text_digest(size_t a_at, uint64_t n, uint64_t first, uint64_t acc[3]) = 0;
    virtual int combine(uint32_t B, const std::vector<RcJob> &jobs) = 0;                                           // src: offsets in A, out: offsets in O
    virtual int fetch(size_t o_at, uint8_t *h, size_t n) = 0;
    virtual int file_digest(const std::string &path, uint64_t out[3]) = 0;
};

struct HostBackend : RcBackend {
    std::vector<uint8_t> A, O; int fd = -1; std::string name; std::vector<std::pair<uint64_t, uint64_t>> pc;
    ~HostBackend() { close(); }
    int reserve(size_t a, size_t o) override { A.assign(a + 16, 0); O.assign(o + 16, 0); return HARC_AMD_OK; }
    int open(const std::string &path, const std::vector<std::pair<uint64_t, uint64_t>> &pieces) override
    {
        close(); name = path; pc = pieces;
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) { harc_set_error("cannot open %s", path.c_str()); return HARC_AMD_EIO; }
        return HARC_AMD_OK;
    }
    int piece(size_t p, size_t at) override
    {
        size_t got = 0; const size_t n = (size_t)(pc[p].second - pc[p].first);
        while (got < n) { const ssize_t r = pread(fd, A.data() + at + got, n - got, (off_t)(pc[p].first + got)); if (r <= 0) { harc_set_error("short read on %s", name.c_str()); return HARC_AMD_EIO; } got += (size_t)r; }
        return HARC_AMD_OK;
    }
    void close() override { if (fd >= 0) ::close(fd); fd = -1; }
    int upload(size_t at, const uint8_t *h, size_t n) override { memcpy(A.data() + at, h, n); return HARC_AMD_OK; }
    int zero(size_t at, size_t n) override { memset(A.data() + at, 0, n); return HARC_AMD_OK; }
    int digests(bool o, size_t at, uint64_t nblocks, uint32_t B, uint32_t last_len, uint64_t *out) override
    {
        return nblocks ? harc_amd_block_digests_host((o ? O.data() : A.data()) + at, nblocks, B, last_len, out) : HARC_AMD_OK;
    }
    int text_digest(size_t at, uint64_t n, uint64_t first, uint64_t acc[3]) override { ck_digest_host(A.data() + at, n, first, acc); return HARC_AMD_OK; }
    int combine(uint32_t B, const std::vector<RcJob> &jobs) override
    {
        for (const RcJob &J : jobs) {
            std::vector<const uint8_t *> s; std::vector<uint8_t *> q;
            for (uint64_t a : J.src) s.push_back(A.data() + a);
            for (uint64_t a : J.out) q.push_back(O.data() + a);
            rc_combine_host(B, s.data(), (int)s.size(), q.data(), (int)q.size(), J.coef.data());
        }
        return HARC_AMD_OK;
    }
    int fetch(size_t at, uint8_t *h, size_t n) override { memcpy(h, O.data() + at, n); return HARC_AMD_OK; }
    int file_digest(const std::string &path, uint64_t out[3]) override
    {
        std::vector<uint8_t> all;
        if (!slurp_file(path, all, true)) return HARC_AMD_EIO;
        out[0] = out[1] = out[2] = 0;
        ck_digest_host(all.data(), all.size(), 0, out);
        return HARC_AMD_OK;
    }
};

struct DevBackend : RcBackend {
    const harc_amd_params *params; CtxGuard guard; harc_amd_ctx *c = nullptr; DevBuf A{ nullptr }, O{ nullptr }; FileFeeder *feed = nullptr; RingGeom g; std::string name;
    explicit DevBackend(const harc_amd_params *p) : params(p) {}
    ~DevBackend() { close(); if (c) (void)hipStreamSynchronize(c->stream); }     // (A and O go before the context: members are destroyed in reverse order)
    int start(uint64_t largest_file)
    {
        RC_TRY(side_context(params, 100, &guard.c));
        c = guard.c; A.c = c; O.c = c;
        return ring_split(c, 1, 16, "recovery", &g, ring_slice_for(largest_file, 16));
    }
    int reserve(size_t a, size_t o) override { RC_TRY(dev_reserve(&A, a + 16)); return dev_reserve(&O, o + 16); }
    int open(const std::string &path, const std::vector<std::pair<uint64_t, uint64_t>> &pieces) override
    {
        close(); name = path;
        feed = new FileFeeder(c, name.c_str());
        return feed->start(pieces, g);
    }
    int piece(size_t p, size_t at) override { return feed->upload_piece(p, A.p + at, nullptr); }
    void close() override { delete feed; feed = nullptr; }
    int upload(size_t at, const uint8_t *h, size_t n) override { HIP_TRY(hipMemcpyAsync(A.p + at, h, n, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); return HARC_AMD_OK; }
    int zero(size_t at, size_t n) override { if (n) HIP_TRY(hipMemsetAsync(A.p + at, 0, n, c->stream)); return HARC_AMD_OK; }
    int digests(bool o, size_t at, uint64_t nblocks, uint32_t B, uint32_t last_len, uint64_t *out) override { return rc_digests_launch(c, (o ? O.p : A.p) + at, nblocks, B, last_len, out); }
    int text_digest(size_t at, uint64_t n, uint64_t first, uint64_t acc[3]) override { return harc_amd_text_digest_device(c, A.p + at, n, first, acc); }
    int combine(uint32_t B, const std::vector<RcJob> &jobs) override
    {
        std::vector<RcJob> abs(jobs);
        for (RcJob &J : abs) { for (uint64_t &a : J.src) a += (uint64_t)(uintptr_t)A.p; for (uint64_t &a : J.out) a += (uint64_t)(uintptr_t)O.p; }
        return rc_combine_launch(c, B, abs);
    }
    int fetch(size_t at, uint8_t *h, size_t n) override { HIP_TRY(hipMemcpyAsync(h, O.p + at, n, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); return HARC_AMD_OK; }
    int file_digest(const std::string &path, uint64_t out[3]) override { return harc_amd_text_digest_files(params, path.c_str(), out); }
};

// ------------------------------------------------------------------------------------------------ the driver
static std::string rc_basename(const std::string &p) { const size_t k = p.rfind('/'); return k == std::string::npos ? p : p.substr(k + 1); }
static std::string rc_dirname(const std::string &p) { const size_t k = p.rfind('/'); return k == std::string::npos ? std::string(".") : k == 0 ? std::string("/") : p.substr(0, k); }
static bool rc_pwrite(int fd, const uint8_t *p, size_t n, uint64_t off)
{
    size_t put = 0;
    while (put < n) { const ssize_t r = pwrite(fd, p + put, n - put, (off_t)(off + put)); if (r <= 0) return false; put += (size_t)r; }
    return true;
}
static bool rc_pread(int fd, uint8_t *p, size_t n, uint64_t off)
{
    size_t got = 0;
    while (got < n) { const ssize_t r = pread(fd, p + got, n - got, (off_t)(off + got)); if (r <= 0) return false; got += (size_t)r; }
    return true;
}
struct FdGuard { int fd = -1; ~FdGuard() { if (fd >= 0) ::close(fd); } };
// block_bytes, span_blocks, group_blocks: 0 = HARC_AMD_RECOVERY_BLOCK / _SPAN / _GROUP, else the defaults
static int rc_geometry(uint32_t pct, uint32_t B, uint32_t S, uint32_t K, GfGeom *g)
{
    g->B = B ? B : (uint32_t)env_u64("HARC_AMD_RECOVERY_BLOCK", GF_DEFAULT_B);
    g->S = S ? S : (uint32_t)env_u64("HARC_AMD_RECOVERY_SPAN", GF_DEFAULT_S);
    g->K = K ? K : (uint32_t)env_u64("HARC_AMD_RECOVERY_GROUP", GF_MAX_K);
    g->PCT = pct;
    if (!gf_geom_ok(*g) || (uint64_t)g->S * g->B > ((uint64_t)1 << 33)) {
        harc_set_error("recovery record: PCT %u (1 .. 100), blocks of %u bytes (a multiple of 16 from 16 to 2^24), spans of %u blocks (1 .. 2^24, at most 8 GiB), groups of %u blocks (1 .. 128)", g->PCT, g->B, g->S, g->K);
        return HARC_AMD_EINVAL;
    }
    return HARC_AMD_OK;
}
// the spans of a file whose first `bytes` bytes are read
static std::vector<std::pair<uint64_t, uint64_t>> rc_span_pieces(uint64_t bytes, const GfGeom &g)
{
    std::vector<std::pair<uint64_t, uint64_t>> pc;
    const uint64_t sb = (uint64_t)g.S * g.B;
    for (uint64_t a = 0; a < bytes; a += sb) pc.emplace_back(a, bytes - a < sb ? bytes : a + sb);
    return pc;
}

// stats: files, bytes protected, bytes of the record, data blocks, groups
static int rc_make(RcBackend &be, const GfGeom &g, int nfiles, const char *const *paths, const char *out_path, uint64_t stats[5])
{
    std::vector<GfFile> files((size_t)nfiles);
    uint64_t max_a = 0, max_o = 0, R = 0, groups = 0, blocks = 0, bytes = 0;
    for (int f = 0; f < nfiles; f++) {
        GfFile &F = files[(size_t)f];
        F.name = rc_basename(paths[f]);
        if (!gf_name_ok(F.name)) { harc_set_error("recovery_make: '%s' names no file", paths[f]); return HARC_AMD_EINVAL; }
        for (int o = 0; o < f; o++) if (files[(size_t)o].name == F.name) { harc_set_error("recovery_make: two files are named %s", F.name.c_str()); return HARC_AMD_EINVAL; }
        if (!file_size(paths[f], &F.n)) { harc_set_error("cannot open %s", paths[f]); return HARC_AMD_EIO; }
        F.nb = gf_blocks(F.n, g.B); F.rb = gf_file_recovery(F.nb, g);
        F.dd.resize((size_t)F.nb); F.rd.resize((size_t)F.rb);
        const uint32_t s = (uint32_t)(F.nb < g.S ? F.nb : g.S);
        if ((uint64_t)s * g.B > max_a) max_a = (uint64_t)s * g.B;
        if (s && (uint64_t)gf_span_recovery(s, g) * g.B > max_o) max_o = (uint64_t)gf_span_recovery(s, g) * g.B;
        R += F.rb; blocks += F.nb; bytes += F.n;
    }
    const uint64_t hb = gf_head_bytes(files);
    RC_TRY(be.reserve((size_t)max_a, (size_t)max_o));
    OutFileGuard og{ out_path };
    FdGuard o;
    o.fd = ::open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (o.fd < 0) { harc_set_error("cannot create %s", out_path); return HARC_AMD_EIO; }
    std::vector<uint8_t> hbuf;
    uint64_t roff = hb;
    for (int f = 0; f < nfiles; f++) {
        GfFile &F = files[(size_t)f];
        if (!F.n) continue;
        uint64_t T[3] = { 0, 0, 0 }, rbase = 0;
        const std::vector<std::pair<uint64_t, uint64_t>> pc = rc_span_pieces(F.n, g);
        RC_TRY(be.open(paths[f], pc));
        for (size_t sp = 0; sp < pc.size(); sp++) {
            const uint64_t len = pc[sp].second - pc[sp].first;
            const uint32_t s = gf_span_blocks(F.nb, g.S, sp), G = gf_groups(s, g.K), last = (uint32_t)(len - (uint64_t)(s - 1) * g.B);
            RC_TRY(be.piece(sp, 0));
            RC_TRY(be.zero((size_t)len, (size_t)((uint64_t)s * g.B - len)));                                        // the last block is padded for the arithmetic only
            RC_TRY(be.digests(false, 0, s, g.B, last, &F.dd[sp * (size_t)g.S]));
            RC_TRY(be.text_digest(0, len, pc[sp].first, T));
            std::vector<RcJob> jobs(G);
            uint32_t r = 0;
            for (uint32_t q = 0; q < G; q++) {
                const uint32_t k = gf_group_members(s, G, q), m = gf_group_recovery(k, g.PCT);
                RcJob &J = jobs[q];
                for (uint32_t j = 0; j < k; j++) J.src.push_back((uint64_t)(j * G + q) * g.B);
                for (uint32_t i = 0; i < m; i++) J.out.push_back((uint64_t)(r + i) * g.B);
                J.coef.resize((size_t)m * k);
                for (uint32_t i = 0; i < m; i++) for (uint32_t j = 0; j < k; j++) J.coef[(size_t)i * k + j] = (uint8_t)gf_cauchy(i, j);
                r += m;
            }
            groups += G;
            RC_TRY(be.combine(g.B, jobs));
            RC_TRY(be.digests(true, 0, r, g.B, g.B, &F.rd[(size_t)rbase]));
            hbuf.resize((size_t)r * g.B);
            RC_TRY(be.fetch(0, hbuf.data(), hbuf.size()));
            if (!rc_pwrite(o.fd, hbuf.data(), hbuf.size(), roff)) { harc_set_error("short write on %s", out_path); return HARC_AMD_EIO; }
            roff += hbuf.size(); rbase += r;
        }
        be.close();
        if (T[0] != F.n || rbase != F.rb) { harc_set_error("recovery_make: %s changed while it was read", paths[f]); return HARC_AMD_EIO; }
        F.D = T[2];
    }
    const std::vector<uint8_t> head = gf_head_build(g, files);
    uint8_t tail[8];
    for (int k = 0; k < 8; k++) tail[k] = (uint8_t)(hb >> (8 * k));
    if (head.size() != hb || roff != hb + R * g.B) { harc_set_error("recovery_make: the record's bookkeeping does not add up"); return HARC_AMD_EINTERNAL; }
    if (!rc_pwrite(o.fd, head.data(), head.size(), 0) || !rc_pwrite(o.fd, head.data(), head.size(), roff) || !rc_pwrite(o.fd, tail, 8, roff + hb) || fsync(o.fd) != 0) {
        harc_set_error("short write on %s", out_path); return HARC_AMD_EIO; }
    if (stats) { stats[0] = (uint64_t)nfiles; stats[1] = bytes; stats[2] = gf_record_bytes(hb, R, g.B); stats[3] = blocks; stats[4] = groups; }
    og.ok = true;
    return HARC_AMD_OK;
}

static void rc_line(std::string *rep, const char *fmt, ...)
{
    char b[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    *rep += "[recovery] "; *rep += b; *rep += "\n";
}
// write == 0: report alone.  *status: 0 when every named file verifies in the end (write == 0: when nothing at all is damaged), else 1
static int rc_repair(RcBackend &be, const char *record_path, int write, std::string *rep, int32_t *status)
{
    *status = 1;
    uint64_t rsize = 0;
    const std::string rname = rc_basename(record_path), dir = rc_dirname(record_path);
    if (!file_size(record_path, &rsize)) { harc_set_error("%s is missing: the archive was not compressed with -P", record_path); return HARC_AMD_EIO; }
    FdGuard rf;
    rf.fd = ::open(record_path, O_RDONLY);
    if (rf.fd < 0) { harc_set_error("cannot open %s", record_path); return HARC_AMD_EIO; }
    GfHead H; int which = 0; std::string why;
    if (!gf_head_find([&](uint64_t off, uint64_t n, uint8_t *dst) { return rc_pread(rf.fd, dst, (size_t)n, off); }, rsize, &H, &which, &why)) {
        harc_set_error("%s: %s", record_path, why.c_str()); return HARC_AMD_EINVAL; }
    const GfGeom g = H.g;
    const size_t nf = H.files.size();
    // what is there of every file; a longer file is refused before anything is read or written
    std::vector<std::string> path(nf); std::vector<uint64_t> have(nf, 0), pb(nf, 0); std::vector<char> missing(nf, 0);
    uint64_t max_a = (uint64_t)2 * GF_MAX_K * g.B;
    for (size_t f = 0; f < nf; f++) {
        const GfFile &F = H.files[f];
        path[f] = dir + "/" + F.name;
        uint64_t fsz = 0;
        struct stat st;
        if (stat(path[f].c_str(), &st) != 0) missing[f] = 1;
        else if (!file_size(path[f].c_str(), &fsz)) { harc_set_error("%s is no regular file", path[f].c_str()); return HARC_AMD_EINVAL; }
        if (fsz > F.n) { harc_set_error("%s holds %llu bytes, %s records %llu: a file that grew is not repaired (inserted bytes shift every block); nothing was written", path[f].c_str(),
                                        (unsigned long long)fsz, rname.c_str(), (unsigned long long)F.n); return HARC_AMD_EINVAL; }
        pb[f] = fsz == F.n ? F.nb : fsz / g.B;                    // whole blocks that are there; a cut block is lost
        have[f] = fsz == F.n ? F.n : pb[f] * g.B;
        const uint64_t s = F.nb < g.S ? F.nb : g.S;
        if (s * g.B > max_a) max_a = s * g.B;
    }
    { const uint64_t s = H.recovery_blocks < g.S ? H.recovery_blocks : g.S; if (s * g.B > max_a) max_a = s * g.B; }
    RC_TRY(be.reserve((size_t)max_a, (size_t)GF_MAX_K * g.B));
    // ---- pass 1: the digest of every block that is there, against the record
    std::vector<std::vector<char>> bad(nf), rbad(nf);
    uint64_t rdamaged = 0, roff = H.head_bytes;
    std::vector<uint64_t> dg;
    for (size_t f = 0; f < nf; f++) {
        const GfFile &F = H.files[f];
        bad[f].assign((size_t)F.nb, 1); rbad[f].assign((size_t)F.rb, 1);
        if (have[f]) {
            const std::vector<std::pair<uint64_t, uint64_t>> pc = rc_span_pieces(have[f], g);
            RC_TRY(be.open(path[f], pc));
            for (size_t sp = 0; sp < pc.size(); sp++) {
                const uint64_t len = pc[sp].second - pc[sp].first, s = gf_blocks(len, g.B);
                RC_TRY(be.piece(sp, 0));
                dg.resize((size_t)s);
                RC_TRY(be.digests(false, 0, s, g.B, (uint32_t)(len - (s - 1) * g.B), dg.data()));
                for (uint64_t t = 0; t < s; t++) bad[f][(size_t)(sp * g.S + t)] = dg[(size_t)t] != F.dd[(size_t)(sp * g.S + t)];
            }
            be.close();
        }
        if (F.rb) {
            std::vector<std::pair<uint64_t, uint64_t>> pc = rc_span_pieces(F.rb * g.B, g);
            for (auto &p : pc) { p.first += roff; p.second += roff; }
            RC_TRY(be.open(record_path, pc));
            for (size_t sp = 0; sp < pc.size(); sp++) {
                const uint64_t s = (pc[sp].second - pc[sp].first) / g.B;
                RC_TRY(be.piece(sp, 0));
                dg.resize((size_t)s);
                RC_TRY(be.digests(false, 0, s, g.B, g.B, dg.data()));
                for (uint64_t t = 0; t < s; t++) { const bool b = dg[(size_t)t] != F.rd[(size_t)(sp * g.S + t)]; rbad[f][(size_t)(sp * g.S + t)] = b; rdamaged += b; }
            }
            be.close();
        }
        roff += F.rb * g.B;
    }
    bool all_ok = true, record_ok = which == 1 && !rdamaged;
    if (which == 2) rc_line(rep, "%s: the first copy of the head is damaged, the second holds", rname.c_str());
    if (rdamaged) rc_line(rep, "%s: %llu of %llu recovery blocks damaged", rname.c_str(), (unsigned long long)rdamaged, (unsigned long long)H.recovery_blocks);
    // ---- pass 2: the groups that lost something
    roff = H.head_bytes;
    std::vector<uint8_t> hbuf, obuf;
    for (size_t f = 0; f < nf; roff += H.files[f].rb * g.B, f++) {
        const GfFile &F = H.files[f];
        uint64_t lost = 0;
        for (char b : bad[f]) lost += b;
        if (!lost && !missing[f]) { rc_line(rep, "%s ok", F.name.c_str()); continue; }
        // can every group be solved?  Nothing of the file is written otherwise
        struct Fix { uint64_t sp; uint32_t G, q, k; uint64_t rbase; std::vector<uint32_t> lost, rec; };
        std::vector<Fix> fixes;
        bool solvable = true;
        uint64_t rbase = 0;
        for (uint64_t sp = 0; sp < gf_spans(F.nb, g.S) && solvable; sp++) {
            const uint32_t s = gf_span_blocks(F.nb, g.S, sp), G = gf_groups(s, g.K);
            for (uint32_t q = 0; q < G; q++) {
                const uint32_t k = gf_group_members(s, G, q), m = gf_group_recovery(k, g.PCT);
                Fix X{ sp, G, q, k, rbase, {}, {} };
                for (uint32_t j = 0; j < k; j++) if (bad[f][(size_t)(sp * g.S + (uint64_t)j * G + q)]) X.lost.push_back(j);
                uint32_t intact = 0;
                for (uint32_t i = 0; i < m; i++) if (!rbad[f][(size_t)(rbase + i)]) { intact++; if (X.rec.size() < X.lost.size()) X.rec.push_back(i); }
                rbase += m;
                if (X.lost.empty()) continue;
                if (X.lost.size() > intact) {
                    rc_line(rep, "%s NOT recoverable: span %llu group %u has lost %zu of %u blocks and holds %u recovery blocks", F.name.c_str(), (unsigned long long)sp, q, X.lost.size(), k, intact);
                    solvable = false; break;
                }
                fixes.push_back(X);
            }
        }
        if (!solvable) { all_ok = false; continue; }
        if (!write) { all_ok = false; rc_line(rep, "%s damaged: %llu of %llu blocks, recoverable", F.name.c_str(), (unsigned long long)lost, (unsigned long long)F.nb); continue; }
        FdGuard df;
        df.fd = ::open(path[f].c_str(), O_RDWR | O_CREAT, 0644);
        if (df.fd < 0) { harc_set_error("cannot open %s for writing", path[f].c_str()); return HARC_AMD_EIO; }
        bool wrong = false;
        for (const Fix &X : fixes) {
            const int e = (int)X.lost.size();
            const uint64_t t0 = X.sp * g.S;
            RcJob J;
            hbuf.assign((size_t)X.k * g.B, 0);
            uint32_t slot = 0; size_t nl = 0;
            for (uint32_t j = 0; j < X.k; j++) {                  // the intact members, in ascending order; the file's last block is padded with zeros
                if (nl < X.lost.size() && X.lost[nl] == j) { nl++; continue; }
                const uint64_t t = t0 + (uint64_t)j * X.G + X.q, off = t * g.B, len = F.n - off < g.B ? F.n - off : g.B;
                if (!rc_pread(df.fd, hbuf.data() + (size_t)slot * g.B, (size_t)len, off)) { harc_set_error("short read on %s", path[f].c_str()); return HARC_AMD_EIO; }
                J.src.push_back((uint64_t)slot++ * g.B);
            }
            for (uint32_t i : X.rec) {
                if (!rc_pread(rf.fd, hbuf.data() + (size_t)slot * g.B, g.B, roff + (X.rbase + i) * g.B)) { harc_set_error("short read on %s", record_path); return HARC_AMD_EIO; }
                J.src.push_back((uint64_t)slot++ * g.B);
            }
            for (int q = 0; q < e; q++) J.out.push_back((uint64_t)q * g.B);
            J.coef.resize((size_t)e * X.k);
            if (!gf_repair_coef(X.k, X.lost.data(), X.rec.data(), e, J.coef.data())) { harc_set_error("recovery_repair: a singular matrix in span %llu group %u of %s", (unsigned long long)X.sp, X.q, F.name.c_str()); return HARC_AMD_EINTERNAL; }
            RC_TRY(be.upload(0, hbuf.data(), hbuf.size()));
            RC_TRY(be.combine(g.B, std::vector<RcJob>(1, J)));
            // every rebuilt block against its recorded digest before a byte is written
            const uint64_t tl = t0 + (uint64_t)X.lost.back() * X.G + X.q;
            const uint32_t last_len = (uint32_t)(F.n - tl * g.B < g.B ? F.n - tl * g.B : g.B);
            dg.resize((size_t)e);
            RC_TRY(be.digests(true, 0, (uint64_t)e, g.B, last_len, dg.data()));
            for (int q = 0; q < e; q++) if (dg[(size_t)q] != F.dd[(size_t)(t0 + (uint64_t)X.lost[(size_t)q] * X.G + X.q)]) wrong = true;
            if (wrong) { rc_line(rep, "%s NOT recoverable: span %llu group %u: a rebuilt block does not have its recorded digest", F.name.c_str(), (unsigned long long)X.sp, X.q); break; }
            obuf.resize((size_t)e * g.B);
            RC_TRY(be.fetch(0, obuf.data(), obuf.size()));
            for (int q = 0; q < e; q++) {
                const uint64_t off = (t0 + (uint64_t)X.lost[(size_t)q] * X.G + X.q) * g.B, len = F.n - off < g.B ? F.n - off : g.B;
                if (!rc_pwrite(df.fd, obuf.data() + (size_t)q * g.B, (size_t)len, off)) { harc_set_error("short write on %s", path[f].c_str()); return HARC_AMD_EIO; }
            }
        }
        if (wrong) { all_ok = false; continue; }
        if (fsync(df.fd) != 0) { harc_set_error("cannot sync %s", path[f].c_str()); return HARC_AMD_EIO; }
        uint64_t T[3] = { 0, 0, 0 };
        RC_TRY(be.file_digest(path[f], T));
        if (T[0] != F.n || T[2] != F.D) { all_ok = false; rc_line(rep, "%s NOT recoverable: the repaired file does not have its recorded digest", F.name.c_str()); continue; }
        rc_line(rep, "%s repaired: %llu of %llu blocks", F.name.c_str(), (unsigned long long)lost, (unsigned long long)F.nb);
    }
    *status = all_ok && (write || record_ok) ? 0 : 1;
    return HARC_AMD_OK;
}

static int rc_report_out(const std::string &rep, char *report, uint64_t cap)
{
    if (report && cap) { const size_t n = rep.size() < cap - 1 ? rep.size() : (size_t)(cap - 1); memcpy(report, rep.data(), n); report[n] = 0; }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_recovery_make_host(int32_t n_files, const char *const *paths, uint32_t pct, uint32_t block_bytes, uint32_t span_blocks, uint32_t group_blocks, const char *out_path, uint64_t *stats)
{
    if (n_files < 1 || !paths || !out_path) { harc_set_error("recovery_make_host: bad arguments"); return HARC_AMD_EINVAL; }
    GfGeom g;
    RC_TRY(rc_geometry(pct, block_bytes, span_blocks, group_blocks, &g));
    HostBackend be;
    return rc_make(be, g, n_files, paths, out_path, stats);
}
extern "C" int harc_amd_recovery_repair_host(const char *record_path, int32_t write, char *report, uint64_t report_capacity, int32_t *status)
{
    if (!record_path || !status) { harc_set_error("recovery_repair_host: bad arguments"); return HARC_AMD_EINVAL; }
    HostBackend be; std::string rep;
    const int rc = rc_repair(be, record_path, write, &rep, status);
    rc_report_out(rep, report, report_capacity);
    return rc;
}
extern "C" int harc_amd_recovery_make_files(const harc_amd_params *params, int32_t n_files, const char *const *paths, uint32_t pct, const char *out_path, uint64_t *stats)
{
    if (!params || n_files < 1 || !paths || !out_path) { harc_set_error("recovery_make_files: bad arguments"); return HARC_AMD_EINVAL; }
    GfGeom g;
    RC_TRY(rc_geometry(pct, 0, 0, 0, &g));
    uint64_t largest = 0;
    for (int f = 0; f < n_files; f++) { uint64_t n = 0; if (!paths[f] || !file_size(paths[f], &n)) { harc_set_error("cannot open %s", paths[f] ? paths[f] : "(null)"); return HARC_AMD_EIO; } if (n > largest) largest = n; }
    DevBackend be(params);
    RC_TRY(be.start(largest));
    const double t0 = mono_now();
    const int rc = rc_make(be, g, n_files, paths, out_path, stats);
    if (rc == HARC_AMD_OK && getenv("HARC_AMD_TRACE") && stats) fprintf(stderr, "[recovery] %llu bytes protected in %.3f s\n", (unsigned long long)stats[1], mono_now() - t0);
    return rc;
}
static int rc_repair_files(const harc_amd_params *params, const char *record_path, int write, char *report, uint64_t cap, int32_t *status)
{
    if (!params || !record_path || !status) { harc_set_error("recovery_%s_files: bad arguments", write ? "repair" : "check"); return HARC_AMD_EINVAL; }
    uint64_t rsize = 0;
    *status = 1;
    if (!file_size(record_path, &rsize)) { harc_set_error("%s is missing: the archive was not compressed with -P", record_path); return HARC_AMD_EIO; }
    DevBackend be(params);
    RC_TRY(be.start(rsize * 16));                                 // (the files are larger than their record)
    std::string rep;
    const int rc = rc_repair(be, record_path, write, &rep, status);
    rc_report_out(rep, report, cap);
    return rc;
}
extern "C" int harc_amd_recovery_check_files(const harc_amd_params *params, const char *record_path, char *report, uint64_t report_capacity, int32_t *status)
{
    return rc_repair_files(params, record_path, 0, report, report_capacity, status);
}
extern "C" int harc_amd_recovery_repair_files(const harc_amd_params *params, const char *record_path, char *report, uint64_t report_capacity, int32_t *status)
{
    return rc_repair_files(params, record_path, 1, report, report_capacity, status);
}
