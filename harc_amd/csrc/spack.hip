// spack.hip -- bytes in device memory <-> the packed stream file X.hs (README: "The packed stream file"), what ./harc -c -S writes for the streams of the
// archive and ./harc -d reads.  Every byte of a block is decided by sv_block.h; this file spreads its functions over a workgroup per block, in the way of
// qpack.hip and idpack.hip.
//
// Packing.  Sizes are needed before bytes can be placed: code into scratch, scan, gather.
//   k_sp_encode   a workgroup of 256 per block, lane t owns strand t: the bytes [t q, (t + 1) q) of the block.  One walk forward counts every byte into the
//                 order-0 row (LDS atomics) and every pair into the order-1 table (global atomics: 256 x 256 u32 are 256 KiB, more than the LDS of a CU; the
//                 table stays in L2) and takes the strand's CRC-32; the strand CRCs are combined by multiplication with x^(8 bytes behind).  Lane 0 normalises the order-0
//                 row, lane r row r of the order-1 table; both heads are written into scratch, the rows of mode 2 at their scanned offsets.  Then every lane
//                 codes its strand backwards twice, with either table, into two slabs; the two sums of strand lengths are scanned and sv_choose decides.
//   (scan of the block sizes, prims.hip)
//   k_sp_gather   a workgroup per block writes u32 payload_bytes and the stored text behind its 9 head bytes -- or has the head of the chosen mode and its
//                 strands copied to their byte-granular place by pack_gather_coded (packfile.h).  Nothing outside the blocks is written.
// A lane's walk over its own strand is byte-serial and not coalesced: neighbouring lanes read text q bytes apart, as in idpack.hip (NOTES.md has the rate).
//
// Unpacking.  The block offsets follow from the payload_bytes prefixes (SvRule over sv_prefix, for the walks of packfile.h on the host and in one lane of the device).
//   k_sp_decode   lane 0 validates the head and finds the rows (sv_check_head); a lane per row loads it (mode 1: into LDS, mode 2: into the block's 256 KiB of
//                 scratch), a lane per strand checks its size, decodes forward (sv_strand_decode), writes its bytes and takes their CRC-32.  Any violation
//                 raises the error word: block number << 8 | SV_E_*.
// The drivers are packfile.h's, shared with qpack.hip and idpack.hip: pack_run and pack_device on the way in, which harc_spack_run and harc_amd_spack_device hand
// their scratch, launches, error words and messages; the host call, the run of k_sp_decode, the device call and the file call on the way back, which get SV_FORMAT.
#include "devutil.h"
#include "sv_block.h"
#include "packfile.h"

#define SP_T 256
#define SP_TAB (65536u * 4u)                                       // the order-1 table of a block
#define SP_HEAD1 ((SV_HEAD1_MAX + 15u) & ~15u)
#define SP_HEAD2 ((SV_HEAD2_MAX + 15u) & ~15u)

struct SpShared {
    uint32_t t0[256], crctab[256], rowoff[256];
    uint32_t scan[SP_T / 64 + 1];
    uint32_t crc, want_crc, err, verr, mode, hdr;
    unsigned long long lsum;
};

// scratch of block b at scratch + b * stride: the order-1 table, the head of mode 2, the head of mode 1, 256 slabs of mode 1, 256 of mode 2.
// err[0]: strands that did not fit their slab (never); err[1 + k]: blocks of mode k
__global__ __launch_bounds__(SP_T) void k_sp_encode(const uint8_t *text, uint64_t n, uint32_t B, uint32_t nb, uint8_t *scratch, uint64_t stride, uint32_t slab, uint32_t *bsize,
                                                    uint32_t *bmode, uint32_t *bhead, unsigned int *err)
{
    __shared__ SpShared S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint32_t m = sv_block_text(n, B, b);
    const uint8_t *tx = text + b * (uint64_t)B;
    uint8_t *sc = scratch + b * stride;
    uint32_t *t1 = (uint32_t *)sc;
    uint8_t *head2 = sc + SP_TAB, *head1 = head2 + SP_HEAD2, *slabs = head1 + SP_HEAD1;
    S.t0[t] = 0; S.crctab[t] = im_crc_entry(t);
    for (uint32_t i = t; i < 65536u; i += SP_T) t1[i] = 0;
    if (t == 0) S.crc = 0;
    __syncthreads();
    // ---- the counts and the CRC of strand t
    const uint32_t a0 = sv_strand_at(m, t), ns = sv_strand_bytes(m, t);
    {
        uint32_t prev = 0, c = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < ns; i++) {
            const uint32_t v = tx[a0 + i];
            atomicAdd(&S.t0[v], 1u);
            atomicAdd(&t1[(prev << 8) | v], 1u);
            c = S.crctab[(c ^ v) & 0xFFu] ^ (c >> 8);
            prev = v;
        }
        if (ns) atomicXor(&S.crc, sv_crc_term(c ^ 0xFFFFFFFFu, m, t));
    }
    __syncthreads();
    // ---- the tables
    if (t == 0) (void)id_norm_counts(S.t0, 256u);
    const uint32_t present = (uint32_t)id_norm_counts(t1 + 256u * t, 256u);
    __syncthreads();
    // ---- the two heads
    const uint32_t crc = S.crc;
    uint32_t A0, rows_bytes;
    const uint32_t f0 = S.t0[t] & 0xFFFFu, rank0 = block_excl_scan_u32<SP_T>(f0 != 0, S.scan, &A0);
    const uint32_t rsize = present ? 32u + 2u * sv_row_symbols(t1 + 256u * t) : 0u, roff = block_excl_scan_u32<SP_T>(rsize, S.scan, &rows_bytes);
    const uint32_t h1 = SV_TAB0 + 2u * A0 + SV_LENS, h2 = SV_TAB0 + rows_bytes + SV_LENS;
    if (t == 0) { head1[0] = 1; qv_put32(head1 + 1, m); qv_put32(head1 + 5, crc); head2[0] = 2; qv_put32(head2 + 1, m); qv_put32(head2 + 5, crc); }
    if (t < 32u) { uint32_t bits = 0; for (uint32_t j = 0; j < 8u; j++) bits |= (uint32_t)((S.t0[8u * t + j] & 0xFFFFu) != 0) << j; head1[SV_HEAD0 + t] = (uint8_t)bits; }
    if (f0) { head1[SV_TAB0 + 2u * rank0] = (uint8_t)f0; head1[SV_TAB0 + 2u * rank0 + 1u] = (uint8_t)(f0 >> 8); }
    {
        const unsigned long long pm = __ballot(present != 0);
        if ((t & 63u) == 0) qv_put64(head2 + SV_HEAD0 + 8u * (t >> 6), pm);
    }
    if (present) (void)sv_put_row(head2 + SV_TAB0 + roff, t1 + 256u * t);
    // ---- the strands, both ways
    uint8_t *lo1 = slabs + (uint64_t)t * slab, *lo2 = slabs + (uint64_t)(SV_STRANDS + t) * slab;
    uint32_t len1 = sv_strand_encode(tx + a0, ns, S.t0, 0, lo1, lo1 + slab), len2 = sv_strand_encode(tx + a0, ns, t1, 1, lo2, lo2 + slab);
    if (len1 == QV_SLAB_OVERFLOW || len2 == QV_SLAB_OVERFLOW) { atomicAdd(&err[0], 1u); len1 = len2 = 0; }
    uint32_t total1, total2;
    (void)block_excl_scan_u32<SP_T>(len1, S.scan, &total1);
    (void)block_excl_scan_u32<SP_T>(len2, S.scan, &total2);
    qv_put32(head1 + h1 - SV_LENS + 4u * t, len1);
    qv_put32(head2 + h2 - SV_LENS + 4u * t, len2);
    if (t == 0) {
        const uint32_t md = sv_choose(m, (uint64_t)h1 + total1, (uint64_t)h2 + total2);
        bsize[b] = 4u + (md == 0 ? SV_HEAD0 + m : md == 1u ? h1 + total1 : h2 + total2);
        bmode[b] = md; bhead[b] = md == 1u ? h1 : h2;
        atomicAdd(&err[1u + md], 1u);
    }
}

__global__ __launch_bounds__(SP_T) void k_sp_gather(const uint8_t *text, uint64_t n, uint32_t B, uint32_t nb, const uint8_t *scratch, uint64_t stride, uint32_t slab,
                                                    const uint32_t *bsize, const uint32_t *bmode, const uint32_t *bhead, const uint64_t *boff, uint8_t *out)
{
    __shared__ PackGather S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint32_t m = sv_block_text(n, B, b), md = bmode[b];
    uint8_t *dst = out + boff[b];
    const uint32_t payload = bsize[b] - 4u;
    const uint8_t *sc = scratch + b * stride, *head2 = sc + SP_TAB, *head1 = head2 + SP_HEAD2, *slabs = head1 + SP_HEAD1;
    if (t < 4) dst[t] = (uint8_t)(payload >> (8 * t));
    if (md == 0) {                                                 // stored: the text as it is (byte by byte: nothing outside the caller's text is read)
        const uint8_t *tx = text + b * (uint64_t)B;
        if (t < SV_HEAD0) dst[4 + t] = t ? head1[t] : (uint8_t)0;                            // (both heads hold block_text_bytes and crc32)
        for (uint32_t j = t; j < m; j += SP_T) dst[4u + SV_HEAD0 + j] = tx[j];
        return;
    }
    // the head and the slabs of the chosen mode; the lengths end the head, strand s ends its slab
    const uint8_t *hdr = md == 1u ? head1 : head2, *sl = slabs + (md == 1u ? 0ull : (uint64_t)SV_STRANDS * slab);
    pack_gather_coded(S, dst, payload, hdr, hdr + bhead[b] - SV_LENS, [=](uint32_t s, uint32_t k) { return sl + (uint64_t)(s + 1u) * slab - k; });
}

// blocks: block b of this call at blocks + off[b], off[b + 1] - off[b] bytes with its u32; its text at text + toff[b], toff[b + 1] - toff[b] bytes (the walk has
// held them to the header's block size).  tabs: 256 KiB per block
__global__ __launch_bounds__(SP_T) void k_sp_decode(const uint8_t *blocks, const uint64_t *off, const uint64_t *toff, uint32_t nb, uint8_t *tabs, uint8_t *text, unsigned long long *errw)
{
    __shared__ SpShared S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint8_t *pl = blocks + off[b] + 4;
    const uint32_t pbytes = (uint32_t)(off[b + 1] - off[b] - 4), m = (uint32_t)(toff[b + 1] - toff[b]);
    uint8_t *tx = text + toff[b];
    uint32_t *t1 = (uint32_t *)(tabs + b * (uint64_t)SP_TAB);
    S.crctab[t] = im_crc_entry(t);
    if (t == 0) {
        S.crc = 0; S.lsum = 0; S.verr = SV_E_NONE; S.mode = 0; S.want_crc = 0; S.hdr = 0;
        S.err = (uint32_t)sv_check_head(pl, pbytes, m, &S.mode, &S.want_crc, &S.hdr, S.rowoff);
    }
    __syncthreads();
    if (S.err) { if (t == 0) atomicMin(errw, ((unsigned long long)b << 8) | S.err); return; }
    const uint32_t a0 = sv_strand_at(m, t), ns = sv_strand_bytes(m, t), md = S.mode, hdr = S.hdr;
    if (md == 0) {
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < ns; i++) { const uint32_t v = pl[SV_HEAD0 + a0 + i]; tx[a0 + i] = (uint8_t)v; c = S.crctab[(c ^ v) & 0xFFu] ^ (c >> 8); }
        if (ns) atomicXor(&S.crc, sv_crc_term(c ^ 0xFFFFFFFFu, m, t));
        __syncthreads();
        if (t == 0 && S.crc != S.want_crc) atomicMin(errw, ((unsigned long long)b << 8) | SV_E_CRC);
        return;
    }
    // the smallest code of what is wrong, as sv_block_decode answers
    uint32_t e = SV_E_NONE, len = 0;
    if (md == 1u) { if (t == 0) e = sv_code(sv_load_row(pl + S.rowoff[0], S.t0)); }
    else if (S.rowoff[t]) e = sv_code(sv_load_row(pl + S.rowoff[t], t1 + 256u * t));
    else sv_clear_row(t1 + 256u * t);
    e = id_min(e, sv_code(sv_check_strand(pl, hdr, m, t, &len)));
    if (e != SV_E_NONE) atomicMin(&S.verr, e);
    atomicAdd(&S.lsum, (unsigned long long)len);
    __syncthreads();
    if (t == 0 && S.lsum != pbytes - hdr) S.verr = id_min(S.verr, SV_E_LENGTHS);
    __syncthreads();
    if (S.verr != SV_E_NONE) { if (t == 0) atomicMin(errw, ((unsigned long long)b << 8) | S.verr); return; }
    uint32_t total, c = 0;                                        // (the sum has been checked: the scan stays below 2^32)
    const uint32_t at = block_excl_scan_u32<SP_T>(len, S.scan, &total);
    e = sv_code(sv_strand_decode(pl + hdr + at, len, md == 1u ? S.t0 : t1, md == 2u, tx + a0, ns, S.crctab, &c));
    if (e != SV_E_NONE) atomicMin(&S.verr, e);
    else if (ns) atomicXor(&S.crc, sv_crc_term(c, m, t));
    __syncthreads();
    if (t == 0) {
        if (S.verr != SV_E_NONE) atomicMin(errw, ((unsigned long long)b << 8) | S.verr);
        else if (S.crc != S.want_crc) atomicMin(errw, ((unsigned long long)b << 8) | SV_E_CRC);
    }
}

static const char *sv_error_text(uint32_t e)
{
    switch (e) {
    case 0: return "no device memory for its table";
    case SV_E_MODE: return "its mode is none of 0, 1 and 2";
    case SV_E_SIZE: return "its sizes do not fit its mode or its share of the text";
    case SV_E_BITMAP: return "a bitmap names no symbol";
    case SV_E_ROW: return "a present row of its table does not sum to 4096 or a present symbol has no frequency";
    case SV_E_LENGTHS: return "its strand lengths do not sum to the rest of its payload";
    case SV_E_SHORT: return "a strand with text is shorter than 4 bytes, or one without text is not empty";
    case SV_E_TRUNC: return "a strand ends before its last byte";
    case SV_E_CONTEXT: return "a byte is coded in a row that is absent or in a slot that is empty";
    case SV_E_END: return "a strand does not end in the state and at the byte it must";
    case SV_E_CRC: return "the CRC-32 of its text is not the one it carries";
    }
    return "unknown error";
}

// ------------------------------------------------------------------------------------------------ packing: the blocks of n bytes
static int sp_check_block(const char *who, uint32_t *B)
{
    if (*B == 0) *B = SV_DEFAULT_B;
    if (*B > SV_MAX_B) { harc_set_error("%s: %u text bytes per block are more than %u", who, *B, SV_MAX_B); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}
// the blocks alone (no file header) -> d_out[0 .. *n_out); d_out == nullptr: the size alone
static int harc_spack_run(harc_amd_ctx *c, const uint8_t *d_text, uint64_t n, uint32_t B, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out, PackStats *st)
{
    const uint32_t mmax = n < B ? (uint32_t)n : B, slab = sv_slab_bytes(mmax);
    const uint64_t stride = (uint64_t)SP_TAB + SP_HEAD2 + SP_HEAD1 + 2ull * SV_STRANDS * slab;
    uint8_t *scratch = nullptr; uint32_t *bhead = nullptr;
    return pack_run(c, "spack", sv_blocks(n, B), 0x7FFFFFF0ull, n, d_out, out_capacity, n_out, st,
        [&](const PackBlocks &P) -> int { RC_TRY(dalloc(c, &scratch, (size_t)(stride * P.nb))); return dalloc(c, &bhead, (size_t)P.nb); },
        [&](const PackBlocks &P) { hipLaunchKernelGGL(k_sp_encode, harc_fold256(P.nb), dim3(SP_T), 0, c->stream, d_text, n, B, P.nb, scratch, stride, slab, P.bsize, P.bmode, bhead, P.err); },
        [&](const unsigned int *err, PackStats *stats) {
            if (err[0]) { harc_set_error("spack: %u strands did not fit their scratch", err[0]); return HARC_AMD_EINTERNAL; }
            if (stats) for (int k = 0; k < 3; k++) stats->mode[k] += err[1 + k];
            return HARC_AMD_OK;
        },
        [&](const PackBlocks &P, uint8_t *out) {
            hipLaunchKernelGGL(k_sp_gather, harc_fold256(P.nb), dim3(SP_T), 0, c->stream, d_text, n, B, P.nb, (const uint8_t *)scratch, stride, slab, (const uint32_t *)P.bsize,
                               (const uint32_t *)P.bmode, (const uint32_t *)bhead, (const uint64_t *)P.boff, out);
        });
}

extern "C" uint64_t harc_amd_spack_bound(uint64_t text_bytes, uint32_t block_bytes) { return sv_bound(text_bytes, block_bytes ? block_bytes : SV_DEFAULT_B); }

extern "C" int harc_amd_spack_device(harc_amd_ctx *c, const uint8_t *d_text, uint64_t text_bytes, uint32_t block_bytes, int32_t flags, uint8_t *d_out, uint64_t out_capacity,
                                     uint64_t *n_out)
{
    uint32_t B = block_bytes;
    return pack_device("spack", c, !text_bytes || d_text, (flags & 1) ? SV_FILE_HEADER : 0, d_out, out_capacity, n_out,
        [&] { return sp_check_block("spack_device", &B); },
        [&](uint8_t *o, uint64_t cap, uint64_t *nblk, PackStats *st) { return harc_spack_run(c, d_text, text_bytes, B, o, cap, nblk, st); },
        [&](uint8_t *h) { sv_file_header(h, B, text_bytes); },
        [&](const PackStats &st, uint64_t bytes) {
            fprintf(stderr, "[spack] device call: %llu bytes of text -> %llu bytes in %llu blocks (%llu stored, %llu order 0, %llu order 1), kernels %.3f ms (%.2f GB/s of text)\n",
                    (unsigned long long)text_bytes, (unsigned long long)bytes, (unsigned long long)st.blocks, (unsigned long long)st.mode[0], (unsigned long long)st.mode[1],
                    (unsigned long long)st.mode[2], 1e3 * st.seconds, st.seconds > 0 ? 1e-9 * (double)st.text / st.seconds : 0.0);
        });
}

// ------------------------------------------------------------------------------------------------ unpacking
// the 32 bytes at h of a packed form of n_bytes bytes.  H->n: the text bytes, H->rb: those of a block, so that pack_block_lines is a block's share of the text
static int sp_parse_header(const char *who, const uint8_t *h, uint64_t n_bytes, PackHeader *H)
{
    if (!sv_magic_ok(h)) { harc_set_error("%s: no packed stream file: its first 8 bytes are not the magic HARCS1", who); return HARC_AMD_EINVAL; }
    H->L = 0; H->rb = qv_le32(h + 8); H->n = qv_le64(h + 16); H->text = H->n;
    if (qv_le32(h + 12) || qv_le64(h + 24)) { harc_set_error("%s: bytes 12..15 or 24..31 of the header are not 0", who); return HARC_AMD_EINVAL; }
    if (H->n == 0) {
        if (H->rb || n_bytes != SV_FILE_HEADER) { harc_set_error("%s: the header announces no text, but a block size or %llu bytes behind it", who, (unsigned long long)(n_bytes - SV_FILE_HEADER)); return HARC_AMD_EINVAL; }
        H->nb = 0;
        return HARC_AMD_OK;
    }
    if (H->rb < 1 || H->rb > SV_MAX_B) { harc_set_error("%s: the header names %u text bytes per block", who, H->rb); return HARC_AMD_EINVAL; }
    H->nb = sv_blocks(H->n, H->rb);
    if (H->nb > (n_bytes - SV_FILE_HEADER) / SV_PREFIX) { harc_set_error("%s: the header announces %llu blocks, %llu bytes cannot hold them", who, (unsigned long long)H->nb, (unsigned long long)n_bytes); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}
// the prefix rule (the text bytes behind the payload bytes of a block are held to its share of the text)
struct SvRule {
    static __host__ __device__ int prefix(const PackHeader &H, uint64_t b, const uint8_t *q, uint64_t left, uint64_t, uint64_t *pb, uint64_t *tb)
    {
        return sv_prefix(q, left, pack_block_lines(H, b), pb, tb);
    }
};
static const PackFormat SV_FORMAT = {
    "s", "stream", "HARC_AMD_SPACK_PIECE", 64, SV_PREFIX, sp_parse_header, SvRule::prefix, pack_walk_device<SvRule>,
    [](harc_amd_ctx *c, const uint8_t *d_blocks, const uint64_t *d_off, const uint64_t *d_toff, uint32_t nb, uint64_t, const PackHeader &, char *d_text, unsigned long long *d_errw) {
        uint8_t *tabs = nullptr;                                   // (inside the pool scope of pack_unpack_run)
        if (dalloc(c, &tabs, (size_t)nb * SP_TAB) != HARC_AMD_OK) { (void)hipMemsetAsync(d_errw, 0, 8, c->stream); return; }      // block 0, code 0
        hipLaunchKernelGGL(k_sp_decode, harc_fold256(nb), dim3(SP_T), 0, c->stream, d_blocks, d_off, d_toff, nb, tabs, (uint8_t *)d_text, d_errw);
    },
    sv_error_text,
};

extern "C" int harc_amd_sunpack_device(harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, uint8_t *d_text, uint64_t out_capacity, uint64_t *n_out)
{
    return pack_unpack_device(SV_FORMAT, c, d_packed, n_bytes, (char *)d_text, out_capacity, n_out);
}

// ------------------------------------------------------------------------------------------------ the same in a row on the host: what the kernels are held to
extern "C" int harc_amd_spack_host(const uint8_t *text, uint64_t text_bytes, uint32_t block_bytes, int32_t flags, uint8_t *out, uint64_t cap, uint64_t *n_out)
{
    if ((text_bytes && !text) || !n_out) { harc_set_error("spack_host: bad arguments"); return HARC_AMD_EINVAL; }
    uint32_t B = block_bytes;
    RC_TRY(sp_check_block("spack_host", &B));
    const uint64_t head = (flags & 1) ? SV_FILE_HEADER : 0;
    std::vector<SvWork> W(1);
    const uint32_t mmax = text_bytes < B ? (uint32_t)text_bytes : B;
    std::vector<uint8_t> slabs((size_t)sv_block_slabs(mmax)), blk;
    uint64_t at = head;
    for (uint64_t a = 0; a < text_bytes; a += B) {
        const uint32_t m = text_bytes - a < B ? (uint32_t)(text_bytes - a) : B;
        blk.resize((size_t)SV_PREFIX + m);
        const uint32_t sz = sv_block_encode(text + a, m, W[0], slabs.data(), blk.data(), blk.size(), nullptr);
        if (!sz) { harc_set_error("spack_host: a strand did not fit its scratch"); return HARC_AMD_EINTERNAL; }
        if (out && at + sz <= cap) memcpy(out + at, blk.data(), sz);
        at += sz;
    }
    *n_out = at;
    if (!out) return HARC_AMD_OK;
    if (cap < at) { harc_set_error("spack_host: the packed form takes %llu bytes, the buffer holds %llu", (unsigned long long)at, (unsigned long long)cap); return HARC_AMD_EINVAL; }
    if (head) sv_file_header(out, B, text_bytes);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_sunpack_host(const uint8_t *packed, uint64_t n_bytes, uint8_t *text, uint64_t cap, uint64_t *n_out)
{
    std::vector<SvWork> W(1);
    return pack_unpack_host(SV_FORMAT, packed, n_bytes, text, cap, n_out,
                            [&](const PackHeader &, const uint8_t *pl, uint32_t pb, uint32_t m, uint8_t *tx) { return sv_block_decode(pl, pb, m, W[0], tx); });
}

// ------------------------------------------------------------------------------------------------ the files
// in_path -> out_path on the context c: the text goes through the feeder's half of the ring in pieces of whole blocks, the packed file through the drain's
static int sp_pack_file(harc_amd_ctx *c, const char *in_path, const char *out_path, size_t slice)
{
    uint64_t isz = 0;
    if (!file_size(in_path, &isz)) { harc_set_error("cannot open %s", in_path); return HARC_AMD_EIO; }
    OutFileGuard outguard{ out_path };
    const uint64_t Benv = env_u64("HARC_AMD_SPACK_BLOCK", SV_DEFAULT_B);
    if (Benv > SV_MAX_B) { harc_set_error("spack_files: HARC_AMD_SPACK_BLOCK=%llu is more than %u", (unsigned long long)Benv, SV_MAX_B); return HARC_AMD_EINVAL; }
    const uint32_t B = (uint32_t)Benv;
    const uint64_t piece_blocks = env_u64(SV_FORMAT.piece_env, SV_FORMAT.piece_default), piece = piece_blocks * B, nb = sv_blocks(isz, B);
    RingGeom g[2];                                                // the feeder's and the drain's
    RC_TRY(ring_split(c, 2, 8, SV_FORMAT.ring, g, slice));
    DevBuf txt{ c }, out{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0;
    PackStats st;
    uint8_t h[SV_FILE_HEADER];
    sv_file_header(h, B, isz);
    uint64_t at = SV_FILE_HEADER; int npieces = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)sv_bound(isz, B), &g[1], true));
        RC_TRY(drain.put_host(h, SV_FILE_HEADER, 0));
        const Pieces pieces = byte_pieces(0, isz, piece);
        FileFeeder feed(c, in_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, g[0]));
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t bytes = pieces[p].second - pieces[p].first;
            RC_TRY(dev_reserve(&txt, (size_t)bytes));
            RC_TRY(dev_reserve(&out, (size_t)(sv_bound(bytes, B) - SV_FILE_HEADER)));
            { const double t0 = mono_now(); RC_TRY(feed.upload_piece(p, txt.p, nullptr)); t_read += mono_now() - t0; }
            uint64_t nblk = 0;
            RC_TRY(harc_spack_run(c, (const uint8_t *)txt.p, bytes, B, (uint8_t *)out.p, out.cap, &nblk, &st));
            { const double t0 = mono_now(); RC_TRY(drain.put(out.p, (size_t)nblk, at)); t_write += mono_now() - t0; }
            at += nblk; npieces++;
        }
        drain.set_final_size(at);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    if (tlog) fprintf(stderr, "[spack] %llu bytes of text -> %llu bytes in %llu blocks (%llu stored, %llu order 0, %llu order 1), %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers\n",
                      (unsigned long long)isz, (unsigned long long)at, (unsigned long long)nb, (unsigned long long)st.mode[0], (unsigned long long)st.mode[1], (unsigned long long)st.mode[2],
                      npieces, st.seconds, t_read, t_write);
    outguard.ok = true;
    return HARC_AMD_OK;
}

// n_files pairs of paths on ONE side context, one after the other; the first failure ends the call (its output is removed, the files in front of it stay).
// The slices of the pinned ring are sized to the largest file, an eighth of it each between 1 and 64 MiB: the streams of a few million reads are a few MB each,
// and pinning the default ring of 1 GiB for them took longer than packing them (NOTES.md)
static int sp_file_list(const char *who, const harc_amd_params *params, int32_t n_files, const char *const *in_paths, const char *const *out_paths, bool unpack)
{
    if (!params || n_files < 0 || (n_files && (!in_paths || !out_paths))) { harc_set_error("%s: bad arguments", who); return HARC_AMD_EINVAL; }
    uint64_t largest = 0;
    for (int32_t k = 0; k < n_files; k++) {
        uint64_t sz = 0;
        if (!in_paths[k] || !out_paths[k]) { harc_set_error("%s: bad arguments", who); return HARC_AMD_EINVAL; }
        if (!file_size(in_paths[k], &sz)) { harc_set_error("cannot open %s", in_paths[k]); return HARC_AMD_EIO; }       // before a device is touched
        if (sz > largest) largest = sz;
    }
    if (!n_files) return HARC_AMD_OK;
    size_t slice = (size_t)1 << 20;
    while (slice < ((size_t)64 << 20) && slice * 8 < largest) slice <<= 1;
    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    for (int32_t k = 0; k < n_files; k++)
        RC_TRY(unpack ? pack_unpack_files(SV_FORMAT, params, in_paths[k], out_paths[k], guard.c, slice) : sp_pack_file(guard.c, in_paths[k], out_paths[k], slice));
    return HARC_AMD_OK;
}
extern "C" int harc_amd_spack_file_list(const harc_amd_params *params, int32_t n_files, const char *const *in_paths, const char *const *out_paths)
{
    return sp_file_list("spack_file_list", params, n_files, in_paths, out_paths, false);
}
extern "C" int harc_amd_sunpack_file_list(const harc_amd_params *params, int32_t n_files, const char *const *packed_paths, const char *const *out_paths)
{
    return sp_file_list("sunpack_file_list", params, n_files, packed_paths, out_paths, true);
}
extern "C" int harc_amd_spack_files(const harc_amd_params *params, const char *in_path, const char *out_path)
{
    if (!params || !in_path || !out_path) { harc_set_error("spack_files: bad arguments"); return HARC_AMD_EINVAL; }
    return sp_file_list("spack_files", params, 1, &in_path, &out_path, false);
}
extern "C" int harc_amd_sunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path)
{
    if (!params || !packed_path || !out_path) { harc_set_error("sunpack_files: bad arguments"); return HARC_AMD_EINVAL; }
    return sp_file_list("sunpack_files", params, 1, &packed_path, &out_path, true);
}
