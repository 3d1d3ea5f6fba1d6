// prims.hip -- device-wide sort / scan building blocks (rocPRIM).  Everything algorithm-specific is hand-written in
// stage1.hip / stage2.hip; these are the "plain library" pieces (the role std::sort plays at reorder.cpp:305).
#include "devutil.h"
#include <rocprim/rocprim.hpp>

int harc_tmp_reserve(harc_amd_ctx *c, size_t bytes)
{
    if (bytes <= c->tmp_bytes) return HARC_AMD_OK;
    if (c->d_tmp) harc_raw_free(c, c->d_tmp);
    c->d_tmp = nullptr; c->tmp_bytes = 0;
    size_t want = bytes + (bytes >> 3) + 4096;
    RC_TRY(harc_raw_alloc(c, &c->d_tmp, want));
    c->tmp_bytes = want;
    return HARC_AMD_OK;
}

#define PRIM_CALL(call_with_tmp)                                \
    do {                                                        \
        size_t bytes = 0; void *tmp = nullptr;                  \
        HIP_TRY(call_with_tmp);                                 \
        RC_TRY(harc_tmp_reserve(c, bytes));                     \
        tmp = c->d_tmp; bytes = c->tmp_bytes;                   \
        HIP_TRY(call_with_tmp);                                 \
    } while (0)

int prim_sort_pairs_u64_u32(harc_amd_ctx *c, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned end_bit)
{
    if (n == 0) return HARC_AMD_OK;
    if (end_bit > 64) end_bit = 64;
    PRIM_CALL(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0u, end_bit, c->stream));
    return HARC_AMD_OK;
}

int prim_sort_keys_u64(harc_amd_ctx *c, const uint64_t *kin, uint64_t *kout, size_t n, unsigned end_bit)
{
    if (n == 0) return HARC_AMD_OK;
    if (end_bit > 64) end_bit = 64;
    if (end_bit < 1) end_bit = 1;
    PRIM_CALL(rocprim::radix_sort_keys(tmp, bytes, kin, kout, n, 0u, end_bit, c->stream));
    return HARC_AMD_OK;
}

int prim_excl_scan_u32(harc_amd_ctx *c, const uint32_t *in, uint32_t *out, size_t n)
{
    if (n == 0) return HARC_AMD_OK;
    PRIM_CALL(rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    return HARC_AMD_OK;
}

struct u32_to_u64 { __host__ __device__ uint64_t operator()(uint32_t x) const { return (uint64_t)x; } };
struct u8_to_u64 { __host__ __device__ uint64_t operator()(uint8_t x) const { return (uint64_t)x; } };

int prim_excl_scan_u32_to_u64(harc_amd_ctx *c, const uint32_t *in, uint64_t *out, size_t n)
{
    if (n == 0) return HARC_AMD_OK;
    auto it = rocprim::make_transform_iterator(in, u32_to_u64());
    PRIM_CALL(rocprim::exclusive_scan(tmp, bytes, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->stream));
    return HARC_AMD_OK;
}

int prim_excl_scan_u8_to_u64(harc_amd_ctx *c, const uint8_t *in, uint64_t *out, size_t n)
{
    if (n == 0) return HARC_AMD_OK;
    auto it = rocprim::make_transform_iterator(in, u8_to_u64());
    PRIM_CALL(rocprim::exclusive_scan(tmp, bytes, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->stream));
    return HARC_AMD_OK;
}

int prim_incl_scan_u64(harc_amd_ctx *c, const uint64_t *in, uint64_t *out, size_t n)
{
    if (n == 0) return HARC_AMD_OK;
    PRIM_CALL(rocprim::inclusive_scan(tmp, bytes, in, out, n, rocprim::plus<uint64_t>(), c->stream));
    return HARC_AMD_OK;
}

int prim_incl_max_u32(harc_amd_ctx *c, const uint32_t *in, uint32_t *out, size_t n)
{
    if (n == 0) return HARC_AMD_OK;
    PRIM_CALL(rocprim::inclusive_scan(tmp, bytes, in, out, n, rocprim::maximum<uint32_t>(), c->stream));
    return HARC_AMD_OK;
}

// ---- the index build's bins and slots from ONE scan of the sorted keys (harc_dict_build; the linear-probing rule above k_table_place).
// Element i: c = 1 for a head (i == 0 or a key unlike the one before), m = its home slot, -2^62 for any other element.  A part of the sequence sums
// up to c = its heads and m = max over its heads of (home - number of heads before it INSIDE the part): (a, b) -> c = a.c + b.c,
// m = max(a.m, b.m - a.c) -- associative, not commutative.  At head i, with b = c - 1 its bin: binstart[b] = i and
// q[b] = m + n = max over the bins j <= b of (home_j + n - j), what k_table_place turns into slots (q[b] - n + b).
// Reduce, then scan: a wave walks one segment of the keys, 64 at a time, and leaves the segment's part; the library scans the parts (a few
// hundred thousand at most); the same walk again, started from the parts in front of the segment, writes.  28 n bytes; no workgroup waits for
// another.  (rocprim::inclusive_scan over the 16-byte parts with an output iterator that stores at the heads did all of it in one pass and was
// SLOWER than the four passes it replaced -- profiles/README.md, r09.)
struct BinPart { long long m; uint32_t c, pad; };
struct BinPartOp {
    __host__ __device__ BinPart operator()(const BinPart &a, const BinPart &b) const
    {
        const long long bm = b.m - (long long)a.c;
        return BinPart{ a.m > bm ? a.m : bm, a.c + b.c, 0u };
    }
};
#define BINS_NONE (-(1ll << 62))
#define BINS_SEG_MIN 2048u        // keys of a segment, at least; segments are whole multiples of 64 * BINS_UNROLL keys
#define BINS_UNROLL 4             // chunks of 64 keys whose loads are under way together
template <bool WRITE> __global__ __launch_bounds__(256) void k_bins_pass(const uint64_t *k, uint32_t n, uint64_t cap, uint32_t seg, uint32_t nseg, BinPart *part,
                                                                       uint32_t *binstart, uint64_t *q, uint32_t *nbins)
{
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6;   // a wave per segment: everything below is wave-uniform but the lane's own key
    if (w >= nseg) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    uint32_t C = 0; long long M = BINS_NONE;                      // heads so far; WRITE: the max so far, else the lane's own max so far
    if (WRITE) { C = part[w].c; M = part[w].m; }                  // (the parts in front of the segment, scanned)
    const uint64_t base = (uint64_t)w * seg, end = base + seg < n ? base + seg : (uint64_t)n;
    uint64_t carry = base ? k[base - 1] : 0;                      // the key in front of the chunk
    for (uint64_t at = base; at < end; at += 64u * BINS_UNROLL) {
        uint64_t key[BINS_UNROLL];
#pragma unroll
        for (int u = 0; u < BINS_UNROLL; u++) { const uint64_t i = at + 64u * u + lane; key[u] = i < end ? k[i] : 0; }
#pragma unroll
        for (int u = 0; u < BINS_UNROLL; u++) {
            const uint64_t i = at + 64u * u + lane;
            uint64_t prev = __shfl_up(key[u], 1, 64);
            if (lane == 0) prev = carry;
            carry = __shfl(key[u], 63, 64);
            const bool head = i < end && (i == 0 || key[u] != prev);
            const unsigned long long hb = __ballot(head);
            const uint32_t rank = C + (uint32_t)__popcll(hb & below);
            long long v = head ? (long long)bucket_slot(key[u], cap) - (long long)rank : BINS_NONE;
            if (WRITE) {
                for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(v, d, 64); if (lane >= d && o > v) v = o; }
                if (M > v) v = M;
                if (head) { binstart[rank] = (uint32_t)i; q[rank] = (uint64_t)(v + (long long)n); }
                if (i < end && i + 1 == n) *nbins = rank + (head ? 1u : 0u);
                M = __shfl(v, 63, 64);
            } else if (v > M) M = v;
            C += (uint32_t)__popcll(hb);
        }
    }
    if (!WRITE) {
        for (int o = 32; o > 0; o >>= 1) { const long long x = __shfl_xor(M, o, 64); if (x > M) M = x; }
        if (lane == 0) part[w] = BinPart{ M, C, 0u };
    }
}
// scratch: room for the segments' parts, twice; the more of it, the shorter the segments (at least BINS_SEG_MIN keys)
int prim_bins_scan(harc_amd_ctx *c, const uint64_t *skeys, size_t n, uint64_t cap, uint32_t *binstart, uint64_t *q, uint32_t *nbins, void *scratch, size_t scratch_bytes)
{
    if (n == 0) return HARC_AMD_OK;
    const size_t room = scratch_bytes / (2 * sizeof(BinPart));
    if (room == 0 || n > 0xFFFFFFFFull || (n + room - 1) / room > (1u << 30) || room > 0x7FFFFFFFull) { harc_set_error("prim_bins_scan: %zu keys, scratch of %zu bytes", n, scratch_bytes); return HARC_AMD_EINVAL; }
    size_t seg = (n + room - 1) / room;
    if (seg < BINS_SEG_MIN) seg = BINS_SEG_MIN;
    seg = (seg + 64 * BINS_UNROLL - 1) / (64 * BINS_UNROLL) * (64 * BINS_UNROLL);
    const uint32_t nseg = (uint32_t)((n + seg - 1) / seg);       // <= room
    BinPart *part = (BinPart *)scratch, *front = part + nseg;
    const dim3 grid((nseg + 3) / 4);
    hipLaunchKernelGGL(k_bins_pass<false>, grid, dim3(256), 0, c->stream, skeys, (uint32_t)n, cap, (uint32_t)seg, nseg, part, (uint32_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
    PRIM_CALL(rocprim::exclusive_scan(tmp, bytes, part, front, BinPart{ BINS_NONE, 0u, 0u }, (size_t)nseg, BinPartOp(), c->stream));
    hipLaunchKernelGGL(k_bins_pass<true>, grid, dim3(256), 0, c->stream, skeys, (uint32_t)n, cap, (uint32_t)seg, nseg, front, binstart, q, nbins);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}

// ---- stage II's contig structure from ONE scan of flag[] and pos[] (stage2.hip: contig_structure; the definitions stand there).  While no read lies more
// than `cut` reads behind the last head1 (flag '0' or a shard start) before it, the heads ARE the head1, and a part of the reads sums up to c = its
// heads, s = its column steps (L at a head, pos elsewhere; read 0: 0) and last = its last head -- read 0 is a head, so a plain maximum.  Reduce, then
// scan, as k_bins_pass: a wave per segment, 64 reads a trip and CONTIG_UNROLL trips in flight; the library scans the segments' parts; the same walk
// again writes head, cid, gstart and chead, 2 bytes read and 13 written per read.  The write pass also sees every read's distance to its last head1:
// where one is above `cut` it raises info[2], and the caller runs the passes that know the cut instead (what this pass wrote is then wrong past that
// read and is overwritten).  info: [0] contigs, [1] columns, [2] the flag, [3 + e] the column of read e * q.
struct ContigPart { uint64_t s; uint32_t c, last; };
struct ContigPartOp {
    __host__ __device__ ContigPart operator()(const ContigPart &a, const ContigPart &b) const { return ContigPart{ a.s + b.s, a.c + b.c, a.last > b.last ? a.last : b.last }; }
};
#define CONTIG_SEG_MIN 2048u      // reads of a segment, at least; segments are whole multiples of 64 * CONTIG_UNROLL reads
#define CONTIG_SEGS 16384u        // segments of a large input, about
#define CONTIG_UNROLL 4
template <bool WRITE> __global__ __launch_bounds__(256) void k_contig_pass(const uint8_t *flag, const uint8_t *pos, uint32_t n, uint32_t L, uint32_t q, uint32_t cut, uint32_t seg, uint32_t nseg,
                                                                         ContigPart *part, uint8_t *head, uint32_t *cid, uint64_t *gstart, uint32_t *chead, unsigned long long *info)
{
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6;   // a wave per segment: everything below is wave-uniform but the lane's own read
    if (w >= nseg) return;
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long upto = ~0ull >> (63 - lane);        // this lane and the ones below
    uint32_t C = 0, last = 0; uint64_t G = 0;                     // heads, last head and columns so far
    if (WRITE) { C = part[w].c; last = part[w].last; G = part[w].s; }   // (the parts in front of the segment, scanned)
    const uint64_t base = (uint64_t)w * seg, end = base + seg < n ? base + seg : (uint64_t)n;
    uint32_t rem = (uint32_t)(base % q);                          // index of the trip's first read modulo q
    for (uint64_t at = base; at < end; at += 64u * CONTIG_UNROLL) {
        uint8_t f[CONTIG_UNROLL], p[CONTIG_UNROLL];
#pragma unroll
        for (int u = 0; u < CONTIG_UNROLL; u++) { const uint64_t i = at + 64u * u + lane; f[u] = i < end ? flag[i] : (uint8_t)0; p[u] = i < end ? pos[i] : (uint8_t)0; }
#pragma unroll
        for (int u = 0; u < CONTIG_UNROLL; u++) {
            const uint64_t i0 = at + 64u * u, i = i0 + lane;
            const uint32_t m = rem + lane;                        // < q + 64: a shard starts where it is a multiple of q
            const bool sh = q >= 128u ? (m == 0 || m == q) : (m % q) == 0;
            if (q >= 128u) { rem += 64u; if (rem >= q) rem -= q; } else rem = (rem + 64u) % q;
            const bool h = i < end && (f[u] == '0' || sh);
            const unsigned long long hb = __ballot(h);
            uint32_t v = i >= end ? 0u : h ? (i == 0 ? 0u : L) : (uint32_t)p[u];   // a trip's steps sum to 64 * 255 at most
            if (WRITE) {
                const uint32_t rank = C + (uint32_t)__popcll(hb & upto) - (h ? 1u : 0u);
                for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d, 64); if (lane >= (uint32_t)d) v += o; }
                const uint64_t g = G + v;
                const unsigned long long mine = hb & upto;
                const uint32_t l1 = mine ? (uint32_t)i0 + 63u - (uint32_t)__clzll(mine) : last;    // the last head1 at or before the read
                if (i < end) {
                    head[i] = h ? 1 : 0; cid[i] = rank; gstart[i] = g;
                    if (h) chead[rank] = (uint32_t)i;
                    if (sh) info[3 + (uint32_t)i / q] = g;
                    if ((uint32_t)i - l1 > cut) info[2] = 1;
                    if (i + 1 == n) { info[0] = rank + (h ? 1u : 0u); info[1] = g + L; }
                }
                G += __shfl(v, 63, 64);
            } else {
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                G += v;
            }
            if (hb) last = (uint32_t)i0 + 63u - (uint32_t)__clzll(hb);
            C += (uint32_t)__popcll(hb);
        }
    }
    if (!WRITE && lane == 0) part[w] = ContigPart{ G, C, last };
}
// head, cid, gstart: n entries; chead: room for n; info (device): 3 + (n - 1) / q + 1 words, the caller reads them behind the stream
int prim_contig_scan(harc_amd_ctx *c, const uint8_t *flag, const uint8_t *pos, size_t n, uint32_t L, uint32_t q, uint32_t cut, uint8_t *head, uint32_t *cid, uint64_t *gstart,
                     uint32_t *chead, unsigned long long *info)
{
    if (n == 0) return HARC_AMD_OK;
    if (n > 0xFFFFFFFFull || q == 0) { harc_set_error("prim_contig_scan: %zu reads, shards of %u", n, q); return HARC_AMD_EINVAL; }
    size_t seg = (n + CONTIG_SEGS - 1) / CONTIG_SEGS;
    if (seg < CONTIG_SEG_MIN) seg = CONTIG_SEG_MIN;
    seg = (seg + 64 * CONTIG_UNROLL - 1) / (64 * CONTIG_UNROLL) * (64 * CONTIG_UNROLL);
    const uint32_t nseg = (uint32_t)((n + seg - 1) / seg);
    PoolScope scope(c);
    ContigPart *part = nullptr; RC_TRY(dalloc(c, &part, (size_t)2 * nseg));
    ContigPart *front = part + nseg;
    const dim3 grid((nseg + 3) / 4);
    HIP_TRY(hipMemsetAsync(info + 2, 0, 8, c->stream));
    hipLaunchKernelGGL(k_contig_pass<false>, grid, dim3(256), 0, c->stream, flag, pos, (uint32_t)n, L, q, cut, (uint32_t)seg, nseg, part, (uint8_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr,
                       (uint32_t *)nullptr, (unsigned long long *)nullptr);
    PRIM_CALL(rocprim::exclusive_scan(tmp, bytes, part, front, ContigPart{ 0, 0u, 0u }, (size_t)nseg, ContigPartOp(), c->stream));
    hipLaunchKernelGGL(k_contig_pass<true>, grid, dim3(256), 0, c->stream, flag, pos, (uint32_t)n, L, q, cut, (uint32_t)seg, nseg, front, head, cid, gstart, chead, info);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}

// ---- self-test of the launch geometry (devutil.h: harc_grid256 / harc_gid): n items, a thread each; returns how many were visited and the sum of their
// indices -- n and n (n - 1) / 2 (mod 2^64) when every item was visited exactly once.  tests/test_gpu_parity.py runs it beyond 2^32 items, where a plain
// one-dimensional grid is cut short without an error on this platform.
__global__ void k_selftest_grid(uint64_t n, unsigned long long *out)
{
    const uint64_t i = harc_gid();
    unsigned long long one = i < n ? 1ULL : 0ULL, idx = i < n ? (unsigned long long)i : 0ULL;
    for (int o = 32; o > 0; o >>= 1) { one += __shfl_xor(one, o, 64); idx += __shfl_xor(idx, o, 64); }
    if ((threadIdx.x & 63) == 0 && one) { atomicAdd(&out[0], one); atomicAdd(&out[1], idx); }
}
// ... the same through harc_gid32() (kernels whose item count is a 32-bit number; n < 2^32 only) ...
__global__ void k_selftest_grid32(uint32_t n, unsigned long long *out)
{
    const uint32_t i = harc_gid32();
    unsigned long long one = i < n ? 1ULL : 0ULL, idx = i < n ? (unsigned long long)i : 0ULL;
    for (int o = 32; o > 0; o >>= 1) { one += __shfl_xor(one, o, 64); idx += __shfl_xor(idx, o, 64); }
    if ((threadIdx.x & 63) == 0 && one) { atomicAdd(&out[0], one); atomicAdd(&out[1], idx); }
}
// ... and with FOUR LANES PER ITEM in folded workgroups (harc_fold256 / harc_bid: the geometry of k_orient and k_succ -- 4 n work-items pass 2^32 at a
// quarter of the items): lane 0 of an item's four counts it
__global__ void k_selftest_fold(uint64_t n, unsigned long long *out)
{
    const uint64_t wave = harc_bid() * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint64_t i = wave * 16 + (uint64_t)(lane >> 2);
    const bool mine = i < n && (lane & 3) == 0;
    unsigned long long one = mine ? 1ULL : 0ULL, idx = mine ? (unsigned long long)i : 0ULL;
    for (int o = 32; o > 0; o >>= 1) { one += __shfl_xor(one, o, 64); idx += __shfl_xor(idx, o, 64); }
    if (lane == 0 && one) { atomicAdd(&out[0], one); atomicAdd(&out[1], idx); }
}
extern "C" int harc_amd_selftest_launch(harc_amd_ctx *c, uint64_t n, uint64_t *visited, uint64_t *index_sum)
{
    if (!c || !visited || !index_sum) return HARC_AMD_EINVAL;
    HIP_TRY(hipSetDevice(c->P.device));
    unsigned long long *d = nullptr, h[6] = { 0, 0, 0, 0, 0, 0 };
    HIP_TRY(hipMalloc((void **)&d, sizeof h));
    const bool n32 = n <= 0xFFFFFFFFull;
    hipError_t e = hipMemsetAsync(d, 0, sizeof h, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_selftest_grid, harc_grid256(n), dim3(256), 0, c->stream, n, d); e = hipGetLastError(); }
    if (e == hipSuccess && n32) { hipLaunchKernelGGL(k_selftest_grid32, harc_grid256(n), dim3(256), 0, c->stream, (uint32_t)n, d + 2); e = hipGetLastError(); }
    if (e == hipSuccess) { hipLaunchKernelGGL(k_selftest_fold, harc_fold256((n + 63) / 64), dim3(256), 0, c->stream, n, d + 4); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) { harc_set_error("harc_amd_selftest_launch: %s", hipGetErrorString(e)); return HARC_AMD_ENODEVICE; }
    // the three geometries must agree; the first one that does not is what the caller gets to see
    int k = 0;
    if (n32 && (h[2] != h[0] || h[3] != h[1])) k = 2;
    else if (h[4] != h[0] || h[5] != h[1]) k = 4;
    if (k) harc_set_error("harc_amd_selftest_launch: %s visited %llu items (index sum %llx), the thread-per-item grid %llu (%llx)", k == 2 ? "harc_gid32" : "harc_fold256 / harc_bid", h[k], h[k + 1], h[0], h[1]);
    *visited = h[k]; *index_sum = h[k + 1];
    return k ? HARC_AMD_EINTERNAL : HARC_AMD_OK;
}
