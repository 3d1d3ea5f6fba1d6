// qpack.hip -- quality lines in device memory <-> the packed quality file X.quality.hq (README: "The packed quality file"), what ./harc -c -q -Q writes and
// ./harc -d -q reads.  Every byte of a block is decided by qv_block.h; this file spreads its functions over a workgroup per block.
//
// Packing.  Sizes are needed before bytes can be placed, as in bgzf_out.hip, and the way is the same: code into scratch, scan, gather.
//   k_qp_encode   a workgroup of 256 per block, lane t owns the lines t, t + 256, ... -- which is also strand t.  Pass A: every byte against 33..126, the bitmap,
//                 the stride check.  Pass B: the (A + 1) x A histogram with LDS atomics.  A lane per row normalises it (qv_norm_row) and the table stays in LDS as
//                 frequency | cumulative << 16.  Then every lane codes its strand downwards into its slab of scratch (qv_strand_encode); the strand lengths are
//                 scanned over the workgroup, the header, table and lengths are written in front of the slabs, and the block's size, stored or coded, is decided.
//   (scan of the block sizes, prims.hip)
//   k_qp_gather   a workgroup per block writes u32 payload_bytes and the stored lines without their newlines -- or has head and strands copied to their
//                 byte-granular place by pack_gather_coded (packfile.h).  Nothing outside the blocks is written.
// The lanes of a wave read 64 neighbouring lines at a stride of L + 1 bytes in all three walks over the text: the same cache lines serve the next hundred symbols.
//
// Unpacking.  The block offsets follow from the payload_bytes prefixes (QvRule over qv_prefix, for the walks of packfile.h on the host and in one lane of the device).
//   k_qp_decode   a workgroup per block validates head, table and strand lengths into LDS (qv_check_head, qv_load_row), then a lane per strand decodes forward
//                 (qv_strand_decode) and writes its lines, a newline behind each.  A violation lowers the error word to block number << 8 | the smallest QV_E_* of the block.
// The plumbing of the file calls (probes, guards, ring split, device buffers, kernel timer) is fileio.h's.  The drivers are packfile.h's, shared with idpack.hip and
// spack.hip: pack_run and pack_device on the way in, which harc_qpack_run and harc_amd_qpack_device hand their scratch, launches, error words and messages; the host
// call, the run of k_qp_decode, the device call and the file call on the way back, which get QV_FORMAT.
#include "devutil.h"
#include "qv_block.h"
#include "qm_block.h"
#include "packfile.h"

#define QP_T 256
#define QP_HDR ((14u + 2u * QV_TABLE + 4u * QV_STRANDS + 15u) & ~15u)     // the head of a coded payload in front of the block's slabs, rounded to 16

struct QpShared {
    uint32_t fc[QV_TABLE];
    uint32_t bm[3], bad, A, err, verr, mode;
    uint32_t scan[QP_T / 64 + 1];
    unsigned long long sum;
    uint8_t sym_of[96], byte_of[96];
};

// err[0]: stride positions that hold no newline; err[1]: newlines inside a line; err[2]: strands that did not fit their slab (never); err[3]: stored blocks
__global__ __launch_bounds__(QP_T) void k_qp_encode(const uint8_t *text, uint64_t n_lines, uint32_t L, uint32_t RB, uint32_t nb, uint8_t *scratch, uint64_t stride,
                                                    uint32_t slab, uint32_t *bsize, uint32_t *bmode, unsigned int *err)
{
    __shared__ QpShared S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint64_t line0 = b * (uint64_t)RB;
    const uint32_t m = n_lines - line0 < RB ? (uint32_t)(n_lines - line0) : RB;
    const uint8_t *tx = text + line0 * (L + 1u);
    for (uint32_t i = t; i < QV_TABLE; i += QP_T) S.fc[i] = 0;
    if (t < 3) S.bm[t] = 0;
    if (t == 0) S.bad = 0;
    __syncthreads();
    {   // ---- A: alphabet and stride
        uint64_t lo = 0; uint32_t hi = 0, bad = 0, e0 = 0, e1 = 0;
        for (uint32_t i = t; i < m; i += QP_T) {
            const uint8_t *ln = tx + (uint64_t)i * (L + 1u);
            for (uint32_t j = 0; j < L; j++) {
                const uint32_t v = ln[j], k = v - QV_FIRST;
                if (k < 64u) lo |= 1ull << k; else if (k < QV_MAXA) hi |= 1u << (k - 64u); else { bad = 1; e1 += v == '\n'; }
            }
            e0 += ln[L] != '\n';
        }
        if ((uint32_t)lo) atomicOr(&S.bm[0], (uint32_t)lo);
        if (lo >> 32) atomicOr(&S.bm[1], (uint32_t)(lo >> 32));
        if (hi) atomicOr(&S.bm[2], hi);
        if (bad) atomicOr(&S.bad, 1u);
        if (e0) atomicAdd(&err[0], e0);
        if (e1) atomicAdd(&err[1], e1);
    }
    __syncthreads();
    if (S.bad) {                                                   // a byte outside the alphabet: stored
        if (t == 0) { bsize[b] = 4u + 1u + m * L; bmode[b] = 0; atomicAdd(&err[3], 1u); }
        return;
    }
    const uint32_t A = qv_rank(S.bm, 96);
    if (t < QV_MAXA) qv_map_entry(S.bm, t, S.sym_of, S.byte_of);
    __syncthreads();
    // ---- B: the histogram
    for (uint32_t i = t; i < m; i += QP_T) {
        const uint8_t *ln = tx + (uint64_t)i * (L + 1u);
        uint32_t ctx = A;
        for (uint32_t j = 0; j < L; j++) { const uint32_t y = S.sym_of[ln[j] - QV_FIRST]; atomicAdd(&S.fc[ctx * A + y], 1u); ctx = y; }
    }
    __syncthreads();
    if (t <= A) { qv_norm_row(S.fc + t * A, A); qv_cum_row(S.fc + t * A, A); }
    __syncthreads();
    // ---- the head of the payload: mode, A, bitmap, table
    uint8_t *hdr = scratch + b * stride;
    if (t == 0) { hdr[0] = 1; hdr[1] = (uint8_t)A; qv_put32(hdr + 2, S.bm[0]); qv_put32(hdr + 6, S.bm[1]); qv_put32(hdr + 10, S.bm[2]); }
    for (uint32_t i = t; i < (A + 1u) * A; i += QP_T) { const uint32_t f = S.fc[i] & 0xFFFFu; hdr[14 + 2 * i] = (uint8_t)f; hdr[15 + 2 * i] = (uint8_t)(f >> 8); }
    // ---- the strands
    uint8_t *slab_lo = hdr + QP_HDR + (uint64_t)t * slab;
    uint32_t len = qv_strand_encode(tx, L, m, t, S.fc, A, S.sym_of, slab_lo, slab_lo + slab);
    if (len == QV_SLAB_OVERFLOW) { atomicAdd(&err[2], 1u); len = 0; }
    uint32_t total;
    (void)block_excl_scan_u32<QP_T>(len, S.scan, &total);
    qv_put32(hdr + 14 + 2u * (A + 1u) * A + 4u * t, len);
    if (t == 0) {
        const int coded = qv_use_coded(A, total, m, L);
        bsize[b] = 4u + (coded ? qv_hdr1(A) + total : 1u + m * L);
        bmode[b] = coded ? 1u : 0u;
        if (!coded) atomicAdd(&err[3], 1u);
    }
}

__global__ __launch_bounds__(QP_T) void k_qp_gather(const uint8_t *text, uint64_t n_lines, uint32_t L, uint32_t RB, uint32_t nb, const uint8_t *scratch, uint64_t stride,
                                                    uint32_t slab, const uint32_t *bsize, const uint32_t *bmode, const uint64_t *boff, uint8_t *out)
{
    __shared__ PackGather S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint64_t line0 = b * (uint64_t)RB;
    const uint32_t m = n_lines - line0 < RB ? (uint32_t)(n_lines - line0) : RB;
    uint8_t *dst = out + boff[b];
    const uint32_t payload = bsize[b] - 4u;
    if (t < 4) dst[t] = (uint8_t)(payload >> (8 * t));
    if (!bmode[b]) {
        const uint8_t *tx = text + line0 * (L + 1u);
        if (t == 0) dst[4] = 0;
        for (uint32_t j = t; j < m * L; j += QP_T) { const uint32_t i = j / L; dst[5 + j] = tx[(uint64_t)i * (L + 1u) + (j - i * L)]; }
        return;
    }
    const uint8_t *hdr = scratch + b * stride, *slabs = hdr + QP_HDR;                     // the lengths end the head; strand s ends its slab
    pack_gather_coded(S, dst, payload, hdr, hdr + qv_hdr1(hdr[1]) - 4u * QV_STRANDS, [=](uint32_t s, uint32_t n) { return slabs + (uint64_t)(s + 1u) * slab - n; });
}

// blocks: block b of this call at blocks + off[b], off[b + 1] - off[b] bytes with its u32; lines [b RB, ..) of the n_lines lines at text
__global__ __launch_bounds__(QP_T) void k_qp_decode(const uint8_t *blocks, const uint64_t *off, uint32_t nb, uint64_t n_lines, uint32_t L, uint32_t RB, uint8_t *text,
                                                    unsigned long long *errw)
{
    __shared__ QpShared S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint64_t line0 = b * (uint64_t)RB;
    const uint32_t m = n_lines - line0 < RB ? (uint32_t)(n_lines - line0) : RB;
    const uint8_t *pl = blocks + off[b] + 4;
    const uint32_t pbytes = (uint32_t)(off[b + 1] - off[b] - 4);
    uint8_t *tx = text + line0 * (L + 1u);
    if (t == 0) { S.sum = 0; S.A = 0; S.mode = 0; S.verr = QV_E_NONE; S.err = (uint32_t)qv_check_head(pl, pbytes, m, L, &S.mode, &S.A, S.bm); }
    __syncthreads();
    if (S.err) { if (t == 0) atomicMin(errw, ((unsigned long long)b << 8) | S.err); return; }
    if (S.mode == 0) {
        const uint64_t nbytes = (uint64_t)m * (L + 1u);
        for (uint64_t j = t; j < nbytes; j += QP_T) { const uint64_t i = j / (L + 1u); const uint32_t col = (uint32_t)(j - i * (L + 1u)); tx[j] = col == L ? (uint8_t)'\n' : pl[1 + i * L + col]; }
        return;
    }
    const uint32_t A = S.A, h = qv_hdr1(A), rest = pbytes - h;
    if (t < QV_MAXA) qv_map_entry(S.bm, t, S.sym_of, S.byte_of);
    // the smallest code of what is wrong, as qv_block_decode answers (a length above the rest of the payload is one that the sum will not meet)
    uint32_t e = QV_E_NONE;
    if (t <= A) e = qv_code(qv_load_row(pl + 14, t, A, S.fc + t * A));
    uint32_t len = qv_le32(pl + h - 4u * QV_STRANDS + 4u * t);
    if (qv_strand_lines(m, t) ? len < 4 : len != 0) e = qv_min(e, QV_E_SHORT);
    if (len > rest) { e = qv_min(e, QV_E_LENGTHS); len = 0; }
    if (e != QV_E_NONE) atomicMin(&S.verr, e);
    atomicAdd(&S.sum, (unsigned long long)len);
    __syncthreads();
    if (t == 0 && S.sum != rest) S.verr = qv_min(S.verr, QV_E_LENGTHS);
    __syncthreads();
    if (S.verr != QV_E_NONE) { if (t == 0) atomicMin(errw, ((unsigned long long)b << 8) | S.verr); return; }
    uint32_t total;
    const uint32_t at = block_excl_scan_u32<QP_T>(len, S.scan, &total);
    e = qv_code(qv_strand_decode(pl + h + at, len, S.fc, A, S.byte_of, tx, L, m, t));
    if (e != QV_E_NONE) atomicMin(&S.verr, e);
    __syncthreads();
    if (t == 0 && S.verr != QV_E_NONE) atomicMin(errw, ((unsigned long long)b << 8) | S.verr);
}

static const char *qv_error_text(uint32_t e)
{
    switch (e) {
    case QV_E_MODE: return "its mode is neither 0 nor 1";
    case QV_E_SIZE: return "its payload size does not fit its mode";
    case QV_E_ALPHABET: return "its symbol count is not that of its bitmap";
    case QV_E_ROW: return "a row of its table sums to neither 0 nor 4096";
    case QV_E_LENGTHS: return "its strand lengths do not sum to the rest of its payload";
    case QV_E_SHORT: return "a strand with lines is shorter than 4 bytes, or one without lines is not empty";
    case QV_E_TRUNC: return "a strand ends before its last symbol";
    case QV_E_CONTEXT: return "a symbol is coded in a context that never occurs";
    case QV_E_END: return "a strand does not end in the state and at the byte it must";
    }
    return "unknown error";
}

// ------------------------------------------------------------------------------------------------ packing: the blocks of n lines
static int qp_check_geometry(const char *who, int32_t readlen, uint32_t *rb)
{
    if (readlen < 1 || readlen > 255) { harc_set_error("%s: the read length %d is not in 1..255", who, readlen); return HARC_AMD_EINVAL; }
    if (*rb == 0) *rb = qv_default_rb((uint32_t)readlen);
    if ((uint64_t)*rb * (uint64_t)readlen > QV_MAX_BLOCK_SYMBOLS) { harc_set_error("%s: %u reads of %d per block are more than %u quality values", who, *rb, readlen, QV_MAX_BLOCK_SYMBOLS); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}
// the blocks alone (no file header) -> d_out[0 .. *n_out); d_out == nullptr: the size alone.  Scratch of block b at scratch + b * stride: QP_HDR bytes for the
// head, then a slab per strand
static int harc_qpack_run(harc_amd_ctx *c, const char *d_text, uint64_t n, uint32_t L, uint32_t RB, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out, PackStats *st)
{
    const uint8_t *text = (const uint8_t *)d_text;
    const uint32_t mmax = n < RB ? (uint32_t)n : RB, slab = qv_slab_bytes(qv_strand_lines(mmax, 0) * L);
    const uint64_t stride = (uint64_t)QP_HDR + (uint64_t)QV_STRANDS * slab;
    uint8_t *scratch = nullptr;
    return pack_run(c, "qpack", qv_blocks(n, RB), 0x7FFFFFF0ull, n * (L + 1ull), d_out, out_capacity, n_out, st,
        [&](const PackBlocks &B) { return dalloc(c, &scratch, (size_t)(stride * B.nb)); },
        [&](const PackBlocks &B) { hipLaunchKernelGGL(k_qp_encode, harc_fold256(B.nb), dim3(QP_T), 0, c->stream, text, n, L, RB, B.nb, scratch, stride, slab, B.bsize, B.bmode, B.err); },
        [&](const unsigned int *err, PackStats *stats) {
            if (err[0] || err[1]) {
                harc_set_error("qpack: the text is not lines of %u quality values: %u positions on the %u-byte stride hold no newline and %u newlines are off it", L, err[0], L + 1, err[1]);
                return HARC_AMD_EINVAL;
            }
            if (err[2]) { harc_set_error("qpack: %u strands did not fit their scratch", err[2]); return HARC_AMD_EINTERNAL; }
            if (stats) stats->mode[0] += err[3];
            return HARC_AMD_OK;
        },
        [&](const PackBlocks &B, uint8_t *out) {
            hipLaunchKernelGGL(k_qp_gather, harc_fold256(B.nb), dim3(QP_T), 0, c->stream, text, n, L, RB, B.nb, (const uint8_t *)scratch, stride, slab, (const uint32_t *)B.bsize,
                               (const uint32_t *)B.bmode, (const uint64_t *)B.boff, out);
        });
}

extern "C" uint64_t harc_amd_qpack_bound(uint64_t n_reads, int32_t readlen, uint32_t reads_per_block)
{
    if (readlen < 1 || readlen > 255 || n_reads == 0) return QV_FILE_HEADER;
    return qv_bound(n_reads, (uint32_t)readlen, reads_per_block ? reads_per_block : qv_default_rb((uint32_t)readlen));
}

extern "C" int harc_amd_qpack_device(harc_amd_ctx *c, const char *d_text, uint64_t n_reads, int32_t readlen, uint32_t reads_per_block, int32_t flags, uint8_t *d_out,
                                     uint64_t out_capacity, uint64_t *n_out)
{
    uint32_t rb = reads_per_block;
    return pack_device("qpack", c, !n_reads || d_text, (flags & 1) ? QV_FILE_HEADER : 0, d_out, out_capacity, n_out,
        [&] { return qp_check_geometry("qpack_device", readlen, &rb); },
        [&](uint8_t *o, uint64_t cap, uint64_t *nblk, PackStats *st) { return harc_qpack_run(c, d_text, n_reads, (uint32_t)readlen, rb, o, cap, nblk, st); },
        [&](uint8_t *h) { if (n_reads) qv_file_header(h, (uint32_t)readlen, rb, n_reads); else qv_file_header(h, 0, 0, 0); },
        [&](const PackStats &st, uint64_t bytes) {
            fprintf(stderr, "[qpack] device call: %llu bytes of text -> %llu bytes in %llu blocks (%llu stored), kernels %.3f ms (%.1f GB/s of text)\n", (unsigned long long)st.text,
                    (unsigned long long)bytes, (unsigned long long)st.blocks, (unsigned long long)st.mode[0], 1e3 * st.seconds, st.seconds > 0 ? 1e-9 * (double)st.text / st.seconds : 0.0);
        });
}

// ------------------------------------------------------------------------------------------------ unpacking
// the 32 bytes at h of a packed form of n_bytes bytes
static int qp_parse_header(const char *who, const uint8_t *h, uint64_t n_bytes, PackHeader *H)
{
    if (!qv_magic_ok(h)) { harc_set_error("%s: no packed quality file: its first 8 bytes are not the magic HARCQ1", who); return HARC_AMD_EINVAL; }
    H->L = qv_le32(h + 8); H->rb = qv_le32(h + 12); H->n = qv_le64(h + 16);
    if (H->n == 0) {
        if (H->L || H->rb || n_bytes != QV_FILE_HEADER) { harc_set_error("%s: the header announces no lines, but a read length, a block size or %llu bytes behind it", who, (unsigned long long)(n_bytes - QV_FILE_HEADER)); return HARC_AMD_EINVAL; }
        H->nb = 0; H->text = 0;
        return HARC_AMD_OK;
    }
    if (H->L < 1 || H->L > 255 || H->rb < 1 || (uint64_t)H->rb * H->L > QV_MAX_BLOCK_SYMBOLS) { harc_set_error("%s: the header names a read length of %u and %u reads per block", who, H->L, H->rb); return HARC_AMD_EINVAL; }
    H->nb = qv_blocks(H->n, H->rb);
    if (H->nb > (n_bytes - QV_FILE_HEADER) / 5) { harc_set_error("%s: the header announces %llu blocks, %llu bytes cannot hold them", who, (unsigned long long)H->nb, (unsigned long long)n_bytes); return HARC_AMD_EINVAL; }
    if (H->n > ((uint64_t)1 << 62) / (H->L + 1ull)) { harc_set_error("%s: the header announces %llu lines", who, (unsigned long long)H->n); return HARC_AMD_EINVAL; }
    H->text = H->n * (H->L + 1ull);
    return HARC_AMD_OK;
}
// the prefix rule (the text bytes of a block follow from its number, lines of H.L and their newlines, not from its prefix)
struct QvRule {
    static __host__ __device__ int prefix(const PackHeader &H, uint64_t b, const uint8_t *q, uint64_t left, uint64_t, uint64_t *pb, uint64_t *tb)
    {
        *tb = pack_block_lines(H, b) * (H.L + 1ull);
        return qv_prefix(q, left, pb);
    }
};
static const PackFormat QV_FORMAT = {
    "q", "quality", "HARC_AMD_QPACK_PIECE", 64, QV_PREFIX, qp_parse_header, QvRule::prefix, pack_walk_device<QvRule>,
    [](harc_amd_ctx *c, const uint8_t *d_blocks, const uint64_t *d_off, const uint64_t *, uint32_t nb, uint64_t n, const PackHeader &H, char *d_text, unsigned long long *d_errw) {
        hipLaunchKernelGGL(k_qp_decode, harc_fold256(nb), dim3(QP_T), 0, c->stream, d_blocks, d_off, nb, n, H.L, H.rb, (uint8_t *)d_text, d_errw);
    },
    qv_error_text,
};

extern "C" int harc_amd_qunpack_device(harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, char *d_text, uint64_t out_capacity, uint64_t *n_out)
{
    return pack_unpack_device(QV_FORMAT, c, d_packed, n_bytes, d_text, out_capacity, n_out);
}

// ------------------------------------------------------------------------------------------------ the same in a row on the host: what the kernels are held to
static int qp_host_stride_check(const char *text, uint64_t n, uint32_t L)
{
    uint64_t e0 = 0, e1 = 0;
    for (uint64_t i = 0; i < n; i++) {
        const char *ln = text + i * (L + 1ull);
        for (uint32_t j = 0; j < L; j++) e1 += ln[j] == '\n';
        e0 += ln[L] != '\n';
    }
    if (e0 || e1) {
        harc_set_error("qpack: the text is not lines of %u quality values: %llu positions on the %u-byte stride hold no newline and %llu newlines are off it", L, (unsigned long long)e0, L + 1, (unsigned long long)e1);
        return HARC_AMD_EINVAL;
    }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_qpack_host(const char *text, uint64_t n_reads, int32_t readlen, uint32_t reads_per_block, int32_t flags, uint8_t *out, uint64_t cap, uint64_t *n_out)
{
    if ((n_reads && !text) || !n_out) { harc_set_error("qpack_host: bad arguments"); return HARC_AMD_EINVAL; }
    uint32_t rb = reads_per_block;
    RC_TRY(qp_check_geometry("qpack_host", readlen, &rb));
    const uint32_t L = (uint32_t)readlen;
    RC_TRY(qp_host_stride_check(text, n_reads, L));
    const uint64_t head = (flags & 1) ? QV_FILE_HEADER : 0;
    std::vector<QvWork> W(1);
    const uint32_t mmax = n_reads < rb ? (uint32_t)n_reads : rb;
    std::vector<uint8_t> slabs((size_t)qv_block_slabs(mmax, L)), blk;
    uint64_t at = head;
    for (uint64_t a = 0; a < n_reads; a += rb) {
        const uint32_t m = n_reads - a < rb ? (uint32_t)(n_reads - a) : rb;
        blk.resize((size_t)5 + (size_t)m * L);
        const uint32_t sz = qv_block_encode((const uint8_t *)text + a * (L + 1ull), m, L, W[0], slabs.data(), blk.data(), blk.size(), nullptr);
        if (!sz) { harc_set_error("qpack_host: a strand did not fit its scratch"); return HARC_AMD_EINTERNAL; }
        if (out && at + sz <= cap) memcpy(out + at, blk.data(), sz);
        at += sz;
    }
    *n_out = at;
    if (!out) return HARC_AMD_OK;
    if (cap < at) { harc_set_error("qpack_host: the packed form takes %llu bytes, the buffer holds %llu", (unsigned long long)at, (unsigned long long)cap); return HARC_AMD_EINVAL; }
    if (head) { if (n_reads) qv_file_header(out, L, rb, n_reads); else qv_file_header(out, 0, 0, 0); }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_qunpack_host(const uint8_t *packed, uint64_t n_bytes, char *text, uint64_t cap, uint64_t *n_out)
{
    std::vector<QvWork> W(1);
    return pack_unpack_host(QV_FORMAT, packed, n_bytes, (uint8_t *)text, cap, n_out,
                            [&](const PackHeader &H, const uint8_t *pl, uint32_t pb, uint32_t m, uint8_t *tx) { return qv_block_decode(pl, pb, m, H.L, W[0], tx); });
}

// ------------------------------------------------------------------------------------------------ the files
// map (may be null): every uploaded piece is mapped in place in device memory in front of the coder (qmap.hip); the mapped text never reaches a file
extern "C" int harc_amd_qpack_files_ex(const harc_amd_params *params, const char *quality_path, const char *out_path, const harc_amd_qmap *map, harc_amd_qmap_stats *stats)
{
    if (!params || !quality_path || !out_path) { harc_set_error("qpack_files: bad arguments"); return HARC_AMD_EINVAL; }
    if (map) RC_TRY(harc_qmap_check("qpack_files", map));
    uint64_t qsz = 0;
    if (!file_size(quality_path, &qsz)) { harc_set_error("cannot open %s", quality_path); return HARC_AMD_EIO; }
    OutFileGuard outguard{ out_path };
    // the read length is the length of the first line; everything about the sizes follows from it, before a device is touched
    uint32_t L = 1;
    if (qsz) RC_TRY(first_line_length(quality_path, "qpack_files", &L));
    const uint64_t LL = L + 1ull;
    if (qsz % LL) { harc_set_error("qpack_files: %s holds %llu bytes, no multiple of the %llu bytes of a line of %u quality values and its newline", quality_path, (unsigned long long)qsz, (unsigned long long)LL, L); return HARC_AMD_EINVAL; }
    const uint64_t n = qsz / LL;
    uint32_t rb = (uint32_t)env_u64("HARC_AMD_QPACK_BLOCK", 0);
    RC_TRY(qp_check_geometry("qpack_files", (int32_t)L, &rb));
    const uint64_t piece_blocks = env_u64(QV_FORMAT.piece_env, QV_FORMAT.piece_default), piece_lines = piece_blocks * rb, nb = qv_blocks(n, rb);
    CtxGuard guard;
    RC_TRY(side_context(params, (int)L, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom g[2];                                                // the feeder's and the drain's
    RC_TRY(ring_split(c, 2, 8, QV_FORMAT.ring, g));
    DevBuf txt{ c }, out{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0;
    PackStats st;
    QmAcc acc; qm_acc_zero(&acc);
    double t_map = 0;
    uint8_t h[QV_FILE_HEADER];
    if (n) qv_file_header(h, L, rb, n); else qv_file_header(h, 0, 0, 0);
    uint64_t at = QV_FILE_HEADER; int npieces = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)(n ? qv_bound(n, L, rb) : QV_FILE_HEADER), &g[1], true));
        RC_TRY(drain.put_host(h, QV_FILE_HEADER, 0));
        const Pieces pieces = line_pieces(n, LL, piece_lines);
        FileFeeder feed(c, quality_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, g[0]));
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t bytes = pieces[p].second - pieces[p].first, m = bytes / LL;
            RC_TRY(dev_reserve(&txt, (size_t)bytes));
            RC_TRY(dev_reserve(&out, (size_t)(qv_bound(m, L, rb) - QV_FILE_HEADER)));
            { const double t0 = mono_now(); RC_TRY(feed.upload_piece(p, txt.p, nullptr)); t_read += mono_now() - t0; }
            if (map) RC_TRY(harc_qmap_run(c, txt.p, m, L, map, txt.p, stats ? &acc : nullptr, tlog ? &t_map : nullptr));
            uint64_t nblk = 0;
            RC_TRY(harc_qpack_run(c, txt.p, m, L, rb, (uint8_t *)out.p, out.cap, &nblk, &st));
            { const double t0 = mono_now(); RC_TRY(drain.put(out.p, (size_t)nblk, at)); t_write += mono_now() - t0; }
            at += nblk; npieces++;
        }
        drain.set_final_size(at);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    if (map && stats) qm_acc_stats(&acc, n * (uint64_t)L, stats);
    if (tlog) {
        char mapped[64] = "";
        if (map) snprintf(mapped, sizeof mapped, ", %.3f s in the kernels of the map", t_map);
        fprintf(stderr, "[qpack] %llu bytes of text -> %llu bytes in %llu blocks (%llu stored), %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers%s\n",
                (unsigned long long)qsz, (unsigned long long)at, (unsigned long long)nb, (unsigned long long)st.mode[0], npieces, st.seconds, t_read, t_write, mapped);
    }
    outguard.ok = true;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_qpack_files(const harc_amd_params *params, const char *quality_path, const char *out_path)
{
    return harc_amd_qpack_files_ex(params, quality_path, out_path, nullptr, nullptr);
}

extern "C" int harc_amd_qunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path)
{
    return pack_unpack_files(QV_FORMAT, params, packed_path, out_path);
}

extern "C" int harc_amd_qunpack_range_files(const harc_amd_params *params, const char *packed_path, const char *out_path, uint64_t first_line, uint64_t n_lines)
{
    const uint64_t range[2] = { first_line, n_lines };
    return pack_unpack_files(QV_FORMAT, params, packed_path, out_path, nullptr, 0, range);
}
