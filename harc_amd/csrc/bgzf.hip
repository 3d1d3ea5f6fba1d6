// bgzf.hip -- BGZF (SAM/BAM specification 4.1: gzip members with a BC subfield, at most 64 KiB of text each) in device memory -> its
// text in device memory.  A kernel marks every offset at which a member header parses (candidates: the magic bytes also occur inside
// compressed data); the short candidate list goes to the host, which follows the chain offset + BSIZE + 1 from the first member, O(members),
// so that false candidates never enter it, and uploads one row per member (CDATA, text offset = exclusive scan of ISIZE, ISIZE, CRC).
// Every member is then inflated on its own into its span of the text by the decoder of inflate_member.h, which checks ISIZE and the
// CRC-32 too.  One lane per member, its code tables in a slot of global memory (NOTES.md, BGZF: the shape, what it measures, what is next).
#include "devutil.h"
#include "inflate_member.h"

#define BG_TILE 4096             // candidates counted per 4096 bytes (16 per thread), then written tile by tile
#define BG_SLOTS 262144u         // lanes of the inflate kernel at most (256 CUs x 16 waves at its 4 waves per SIMD): one ImTables slot each

__device__ __forceinline__ bool bg_cand_at(const uint8_t *in, uint64_t n, uint64_t i, BgzfCand *out)
{
    if (i + 18 > n || in[i] != 0x1f || in[i + 1] != 0x8b) return false;
    uint32_t bs = 0, hdr = 0;
    if (!im_bgzf_header(in + i, n - i, &bs, &hdr)) return false;
    if (out) {
        BgzfCand c; c.off = i; c.bsize = bs; c.hdr = hdr; c.crc = 0; c.isize = 0;
        if (i + bs + 1 <= n) { c.crc = im_le32(in + i + bs + 1 - 8); c.isize = im_le32(in + i + bs + 1 - 4); }
        *out = c;
    }
    return true;
}
// candidates in [lo, hi) of in[0 .. n): count per tile
__global__ __launch_bounds__(256) void k_bgzf_cand_count(const uint8_t *in, uint64_t n, uint64_t lo, uint64_t hi, uint64_t ntiles, uint32_t *tilecnt)
{
    __shared__ uint32_t sm[8];
    const uint64_t b = harc_bid();
    if (b >= ntiles) return;
    const uint64_t at = lo + b * BG_TILE + (uint64_t)threadIdx.x * 16;
    uint32_t cnt = 0;
    for (int k = 0; k < 16; k++) if (at + k < hi && bg_cand_at(in, n, at + k, nullptr)) cnt++;
    uint32_t tot; (void)block_excl_scan_u32<256>(cnt, sm, &tot);
    if (threadIdx.x == 0) tilecnt[b] = tot;
}
__global__ __launch_bounds__(256) void k_bgzf_cand_write(const uint8_t *in, uint64_t n, uint64_t lo, uint64_t hi, uint64_t ntiles, const uint64_t *tilebase, BgzfCand *out)
{
    __shared__ uint32_t sm[8];
    const uint64_t b = harc_bid();
    if (b >= ntiles) return;
    const uint64_t at = lo + b * BG_TILE + (uint64_t)threadIdx.x * 16;
    uint32_t m = 0;
    for (int k = 0; k < 16; k++) if (at + k < hi && bg_cand_at(in, n, at + k, nullptr)) m |= 1u << k;
    uint32_t tot; const uint32_t off = block_excl_scan_u32<256>((uint32_t)__popc(m), sm, &tot);
    uint64_t o = tilebase[b] + off;
    while (m) { const int k = __ffs((int)m) - 1; m &= m - 1; bg_cand_at(in, n, at + k, &out[o++]); }
}
// one lane per member, members dealt round robin over at most BG_SLOTS lanes; the first bad member (lowest index) and its IM_E_* code
// end up in *bad as (index << 8 | code)
__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *in, const BgzfMember *mem, uint32_t nm, uint8_t *out, ImTables *tabs, uint32_t nslots,
                                                     unsigned long long *bad)
{
    __shared__ uint32_t crctab[256];
    for (int i = threadIdx.x; i < 256; i += 64) crctab[i] = im_crc_entry((uint32_t)i);
    __syncthreads();
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= nslots) return;
    ImTables &t = tabs[g];
    for (uint32_t i = g; i < nm; i += nslots) {
        const BgzfMember m = mem[i];
        const int rc = im_inflate(in + m.cdata, m.clen, out + m.text, m.isize, m.crc, t, crctab);
        if (rc) atomicMin(bad, ((unsigned long long)i << 8) | (unsigned long long)rc);
    }
}

static const char *im_what(int rc)
{
    switch (rc) {
    case IM_E_TRUNC: return "the DEFLATE data runs past the end of the member";
    case IM_E_BTYPE: return "block type 3";
    case IM_E_STORED: return "stored block length does not match its complement";
    case IM_E_CODES: return "bad Huffman code lengths";
    case IM_E_SYMBOL: return "invalid Huffman code";
    case IM_E_DIST: return "distance before the start of the member";
    case IM_E_OVERFLOW: return "more text than ISIZE";
    case IM_E_SHORT: return "less text than ISIZE";
    case IM_E_CRC: return "CRC-32 mismatch";
    default: return "corrupt member";
    }
}

int harc_bgzf_plan(harc_amd_ctx *c, const uint8_t *d_in, uint64_t n, uint64_t start, uint64_t own_end, uint64_t base_off, BgzfPlan *plan)
{
    plan->m.clear(); plan->text = 0; plan->next = start;
    if (own_end > n) own_end = n;
    if (start >= own_end) return HARC_AMD_OK;
    PoolScope scope(c);
    const uint64_t ntiles = (own_end - start + BG_TILE - 1) / BG_TILE;
    uint32_t *tilecnt = nullptr; uint64_t *tilebase = nullptr;
    RC_TRY(dalloc(c, &tilecnt, (size_t)ntiles + 1)); RC_TRY(dalloc(c, &tilebase, (size_t)ntiles + 1));
    HIP_TRY(hipMemsetAsync(tilecnt + ntiles, 0, 4, c->stream));
    hipLaunchKernelGGL(k_bgzf_cand_count, harc_fold256(ntiles), dim3(256), 0, c->stream, d_in, n, start, own_end, ntiles, tilecnt);
    RC_TRY(prim_excl_scan_u32_to_u64(c, tilecnt, tilebase, (size_t)ntiles + 1));
    uint64_t ncand = 0;
    HIP_TRY(hipMemcpyAsync(&ncand, tilebase + ntiles, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    BgzfCand *d_cand = nullptr; RC_TRY(dalloc(c, &d_cand, (size_t)ncand + 1));
    hipLaunchKernelGGL(k_bgzf_cand_write, harc_fold256(ntiles), dim3(256), 0, c->stream, d_in, n, start, own_end, ntiles, (const uint64_t *)tilebase, d_cand);
    HIP_TRY(hipGetLastError());
    std::vector<BgzfCand> cand((size_t)ncand);
    if (ncand) HIP_TRY(hipMemcpyAsync(cand.data(), d_cand, (size_t)ncand * sizeof(BgzfCand), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the chain: every member starts where the one before it ends; candidates in between are bytes of compressed data
    size_t ci = 0; uint64_t pos = start;
    while (pos < own_end) {
        while (ci < cand.size() && cand[ci].off < pos) ci++;
        if (ci == cand.size() || cand[ci].off != pos) {
            harc_set_error("BGZF: no member header at compressed byte %llu", (unsigned long long)(base_off + pos)); return HARC_AMD_EINVAL;
        }
        const BgzfCand &k = cand[ci];
        if (pos + k.bsize + 1 > n) {
            harc_set_error("BGZF: the member at compressed byte %llu runs past the end of the input (BSIZE %u)", (unsigned long long)(base_off + pos), k.bsize);
            return HARC_AMD_EINVAL;
        }
        if (k.isize > 65536) {
            harc_set_error("BGZF: the member at compressed byte %llu has ISIZE %u > 65536", (unsigned long long)(base_off + pos), k.isize); return HARC_AMD_EINVAL;
        }
        if (plan->m.size() >= 0xFFFFFFF0u) { harc_set_error("BGZF: too many members in one call"); return HARC_AMD_EINVAL; }
        BgzfMember mb; mb.cdata = pos + k.hdr; mb.text = plan->text; mb.clen = k.bsize + 1 - k.hdr - 8; mb.isize = k.isize; mb.crc = k.crc; mb.hdr = k.hdr;
        plan->m.push_back(mb);
        plan->text += k.isize; pos += (uint64_t)k.bsize + 1;
    }
    plan->next = pos;
    return HARC_AMD_OK;
}

int harc_bgzf_run(harc_amd_ctx *c, const uint8_t *d_in, const BgzfPlan &plan, uint64_t base_off, char *d_out)
{
    const uint32_t nm = (uint32_t)plan.m.size();
    if (nm == 0) return HARC_AMD_OK;
    PoolScope scope(c);
    BgzfMember *d_m = nullptr; RC_TRY(dalloc(c, &d_m, (size_t)nm));
    HIP_TRY(hipMemcpyAsync(d_m, plan.m.data(), (size_t)nm * sizeof(BgzfMember), hipMemcpyHostToDevice, c->stream));
    const uint32_t nslots = ((nm < BG_SLOTS ? nm : BG_SLOTS) + 63u) & ~63u;
    ImTables *tabs = nullptr; RC_TRY(dalloc(c, &tabs, (size_t)nslots));
    unsigned long long *d_bad = nullptr; RC_TRY(dalloc(c, &d_bad, 1));
    HIP_TRY(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(nslots / 64), dim3(64), 0, c->stream, d_in, (const BgzfMember *)d_m, nm, (uint8_t *)d_out, tabs, nslots, d_bad);
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad != ~0ull) {
        const BgzfMember &m = plan.m[(size_t)(bad >> 8)];
        harc_set_error("BGZF: the member at compressed byte %llu is corrupt: %s", (unsigned long long)(base_off + m.cdata - m.hdr), im_what((int)(bad & 255)));
        return HARC_AMD_EINVAL;
    }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_bgzf_inflate_device(harc_amd_ctx *c, const uint8_t *d_bgzf, uint64_t n_bytes, char *d_out, uint64_t out_capacity, uint64_t *n_out)
{
    if (!c || (n_bytes && !d_bgzf) || !n_out) { harc_set_error("bgzf_inflate_device: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    BgzfPlan plan;
    RC_TRY(harc_bgzf_plan(c, d_bgzf, n_bytes, 0, n_bytes, 0, &plan));
    *n_out = plan.text;
    if (!d_out) return HARC_AMD_OK;
    if (out_capacity < plan.text) { harc_set_error("bgzf_inflate_device: the text is %llu bytes, the buffer %llu", (unsigned long long)plan.text, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
    return harc_bgzf_run(c, d_bgzf, plan, 0, d_out);
}

extern "C" int harc_amd_set_fastq_bgzf_device(harc_amd_ctx *c, const uint8_t *d_bgzf, uint64_t n_bytes, uint64_t *n_records_out)
{
    if (!c || (n_bytes && !d_bgzf)) { harc_set_error("set_fastq_bgzf_device: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    BgzfPlan plan;
    RC_TRY(harc_bgzf_plan(c, d_bgzf, n_bytes, 0, n_bytes, 0, &plan));
    char *d_txt = nullptr;
    RC_TRY(harc_raw_alloc(c, (void **)&d_txt, (size_t)plan.text + 16));
    struct Free { harc_amd_ctx *c; char *p; ~Free() { harc_raw_free(c, p); } } fr{ c, d_txt };
    RC_TRY(harc_bgzf_run(c, d_bgzf, plan, 0, d_txt));
    return harc_amd_set_fastq_device(c, d_txt, plan.text, n_records_out);
}
