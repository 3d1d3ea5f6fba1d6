// idpack.hip -- an id text in device memory <-> the packed id file X.id.hi (README: "The packed id file"), what ./harc -c -q -I writes and ./harc -d -q
// reads.  Every byte of a block is decided by id_block.h; this file spreads its functions over a workgroup per block, in the way of qpack.hip.
//
// Packing.  Sizes are needed before bytes can be placed: code into scratch, scan, gather.
//   k_ip_encode   a workgroup of 256 per block, lane t owns strand t: the consecutive lines [t q, (t + 1) q) of the block, found through the line index of the
//                 text.  Pass 1: the lane walks its lines forward, tokenising each line and the one in front of it in lockstep straight from the text
//                 (id_strand_events): bytes against 32..126, every event counted into the LDS table with atomics and written as a u16 into the strand's
//                 scratch -- or the strand abandoned at the event bound.  A lane per row normalises; the table stays in LDS as frequency | cumulative << 16.
//                 Pass 2: the lane walks its events backwards through the coder into its slab (id_strand_encode).  The strand lengths are scanned over the
//                 workgroup, the head of the payload is written in front of the table, and the block's size, stored or coded, is decided.
//   (scan of the block sizes, prims.hip)
//   k_ip_gather   a workgroup per block writes u32 payload_bytes and the stored text behind its length -- or has head, table and strands copied to their
//                 byte-granular place by pack_gather_coded (packfile.h).  Nothing outside the blocks is written.
// A lane's walk over its own lines is byte-serial and not coalesced: neighbouring lanes read text q lines apart.  That is accepted here (NOTES.md has the rate).
//
// Unpacking.  The block offsets follow from the payload_bytes prefixes and the places in the text from the block_text_bytes behind them (IdRule over id_prefix,
// for the walks of packfile.h on the host and in one lane of the device).
//   k_ip_decode   a workgroup per block validates head, bitmap, rows and strand sizes into LDS (id_check_head, id_load_row, id_check_strand), then a lane per
//                 strand decodes forward (id_strand_decode) and writes its text at its prefix-summed offset.  Any violation raises the error word:
//                 block number << 8 | ID_E_*.
// The plumbing of the file calls (probes, guards, ring split, device buffers, kernel timer, the carried tail of the text) is fileio.h's.  The drivers are packfile.h's,
// shared with qpack.hip and spack.hip: pack_run and pack_device on the way in, which harc_idpack_run and harc_amd_idpack_device hand their scratch, launches, error
// words and messages (and the line index, built first); the host call, the run of k_ip_decode, the device call and the file call on the way back, which get ID_FORMAT.
#include "devutil.h"
#include "id_block.h"
#include "packfile.h"

#define IP_T 256
#define IP_HDR ((ID_HEAD1 + 2u * ID_TABLE + 15u) & ~15u)          // the head and table of a coded payload, rounded to 16
#define IP_CALL_TEXT ((uint64_t)256 << 20)                        // the file call: text of one kernel call, where more than one block would be more (HARC_AMD_IDPACK_CALL_TEXT in tests)

struct IpShared {
    uint32_t fc[ID_TABLE];
    uint32_t bm[4], present[ID_ROWS], bad, err, verr, mode, tbytes, hdr1, newlines;
    uint32_t scan[IP_T / 64 + 1];
    unsigned long long tsum, lsum;
};

// The blocks of the lines [0, n_lines) whose line index is nls (nls[-1]: the newline in front of the first of them, absolute like the others; t0: where the
// first line starts).  events: u16 (text bytes + 2 lines of the call); slabs: 2 bytes per event and 32 per strand; heads: IP_HDR per block.
// err[0]: 1 + the first block whose text is longer than 2^30 bytes (atomicMin over 0xFFFFFFFF); err[1]: strands that did not fit their slab (never); err[2]: stored blocks
__global__ __launch_bounds__(IP_T) void k_ip_encode(const uint8_t *text, const uint64_t *nls, uint64_t t0, uint64_t n_lines, uint32_t RB, uint32_t nb, uint16_t *events,
                                                    uint8_t *slabs, uint8_t *heads, uint64_t *sat, uint64_t *btext, uint32_t *bsize, uint32_t *bmode, unsigned int *err)
{
    __shared__ IpShared S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint64_t line0 = b * (uint64_t)RB;
    const uint32_t m = n_lines - line0 < RB ? (uint32_t)(n_lines - line0) : RB;
    const uint64_t b0 = nls[(int64_t)line0 - 1] + 1, b1 = nls[line0 + m - 1] + 1;
    if (t == 0) btext[b] = b0;
    if (b1 - b0 > ID_MAX_BLOCK_TEXT) {
        if (t == 0) { atomicMin(&err[0], (unsigned int)b + 1u); bsize[b] = 0; bmode[b] = 0; }
        return;
    }
    const uint32_t T = (uint32_t)(b1 - b0);
    for (uint32_t i = t; i < ID_TABLE; i += IP_T) S.fc[i] = 0;
    if (t == 0) S.bad = 0;
    __syncthreads();
    // ---- pass 1: the events of strand t
    const uint32_t l0 = id_strand_line0(m, t), nl = id_strand_lines(m, t);
    const uint64_t s0 = nls[(int64_t)(line0 + l0) - 1] + 1, s1 = nls[(int64_t)(line0 + l0 + nl) - 1] + 1;
    const uint32_t tb = (uint32_t)(s1 - s0), cap = id_event_cap(tb, nl);
    const uint64_t ev_at = (s0 - t0) + 2ull * (line0 + l0);                                  // in u16
    uint16_t *ev = events + ev_at;
    const uint32_t nev = id_strand_events(text + s0, tb, nl, ev, cap, S.fc);
    if (nev == ID_EV_OVERFLOW || nev == ID_EV_BADBYTE) atomicOr(&S.bad, 1u);
    __syncthreads();
    if (S.bad) {                                                   // a byte outside 32..126 or a strand past the event bound: stored
        if (t == 0) { bsize[b] = 4u + ID_HEAD0 + T; bmode[b] = 0; atomicAdd(&err[2], 1u); }
        return;
    }
    if (t < ID_ROWS) S.present[t] = (uint32_t)id_norm_row(S.fc, t);
    __syncthreads();
    if (t < 4) { uint32_t w = 0; for (uint32_t k = 0; k < 32u && 32u * t + k < ID_ROWS; k++) w |= S.present[32u * t + k] << k; S.bm[t] = w; }
    __syncthreads();
    // ---- the head of the payload: mode, text bytes, strand text bytes, (strand coded bytes below), bitmap, the present rows
    uint8_t *hdr = heads + b * (uint64_t)IP_HDR;
    if (t == 0) { hdr[0] = 1; qv_put32(hdr + 1, T); }
    qv_put32(hdr + ID_HEAD0 + 4u * t, tb);
    if (t < 4) qv_put32(hdr + ID_HEAD1 - 16u + 4u * t, S.bm[t]);
    if (t < ID_ROWS && S.present[t]) {
        uint8_t *o = hdr + ID_HEAD1 + 2u * id_rows_before(S.bm, t);
        const uint32_t *row = S.fc + id_row_off(t);
        for (uint32_t y = 0; y < id_row_width(t); y++) { const uint32_t f = row[y] & 0xFFFFu; o[2 * y] = (uint8_t)f; o[2 * y + 1] = (uint8_t)(f >> 8); }
    }
    // ---- pass 2: the strands
    const uint64_t slab_at = 2ull * ev_at + 32ull * ((uint64_t)ID_STRANDS * b + t);
    uint8_t *slab_lo = slabs + slab_at, *slab_hi = slab_lo + id_slab_bytes(cap);
    uint32_t len = id_strand_encode(ev, nev, S.fc, slab_lo, slab_hi);
    if (len == QV_SLAB_OVERFLOW) { atomicAdd(&err[1], 1u); len = 0; }
    sat[(uint64_t)ID_STRANDS * b + t] = slab_at + id_slab_bytes(cap) - len;
    uint32_t total;
    (void)block_excl_scan_u32<IP_T>(len, S.scan, &total);
    qv_put32(hdr + ID_HEAD0 + 4u * ID_STRANDS + 4u * t, len);
    if (t == 0) {
        const uint32_t hdr1 = ID_HEAD1 + 2u * id_rows_before(S.bm, ID_ROWS);
        const int coded = id_use_coded(hdr1, total, T);
        bsize[b] = 4u + (coded ? hdr1 + total : ID_HEAD0 + T);
        bmode[b] = coded ? 1u : 0u;
        if (!coded) atomicAdd(&err[2], 1u);
    }
}

__global__ __launch_bounds__(IP_T) void k_ip_gather(const uint8_t *text, uint32_t nb, const uint8_t *slabs, const uint8_t *heads, const uint64_t *sat, const uint64_t *btext,
                                                    const uint32_t *bsize, const uint32_t *bmode, const uint64_t *boff, uint8_t *out)
{
    __shared__ PackGather S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    uint8_t *dst = out + boff[b];
    const uint32_t payload = bsize[b] - 4u;
    if (t < 4) dst[t] = (uint8_t)(payload >> (8 * t));
    if (!bmode[b]) {                                               // stored: the text as it is (byte by byte: nothing behind the caller's text is read)
        const uint32_t T = payload - ID_HEAD0;
        const uint8_t *tx = text + btext[b];
        if (t == 0) dst[4] = 0;
        if (t >= 1 && t < 5) dst[4 + t] = (uint8_t)(T >> (8 * (t - 1)));
        for (uint32_t j = t; j < T; j += IP_T) dst[4u + ID_HEAD0 + j] = tx[j];
        return;
    }
    const uint8_t *hdr = heads + b * (uint64_t)IP_HDR;                                       // the lengths follow the strand text bytes; sat says where a strand starts
    const uint64_t *at = sat + (uint64_t)ID_STRANDS * b;
    pack_gather_coded(S, dst, payload, hdr, hdr + ID_HEAD0 + 4u * ID_STRANDS, [=](uint32_t s, uint32_t) { return slabs + at[s]; });
}

// blocks: block b of this call at blocks + off[b], off[b + 1] - off[b] bytes with its u32; its text at text + toff[b], toff[b + 1] - toff[b] bytes (the walk has
// read them from the payload's head and summed them to the size of the text)
__global__ __launch_bounds__(IP_T) void k_ip_decode(const uint8_t *blocks, const uint64_t *off, const uint64_t *toff, uint32_t nb, uint64_t n_lines, uint32_t RB, uint8_t *text,
                                                    unsigned long long *errw)
{
    __shared__ IpShared S;
    const uint64_t b = harc_bid();
    if (b >= nb) return;
    const uint32_t t = threadIdx.x;
    const uint64_t line0 = b * (uint64_t)RB;
    const uint32_t m = n_lines - line0 < RB ? (uint32_t)(n_lines - line0) : RB;
    const uint8_t *pl = blocks + off[b] + 4;
    const uint32_t pbytes = (uint32_t)(off[b + 1] - off[b] - 4);
    uint8_t *tx = text + toff[b];
    if (t == 0) {
        S.tsum = 0; S.lsum = 0; S.verr = ID_E_NONE; S.mode = 0; S.tbytes = 0; S.hdr1 = 0; S.newlines = 0;
        S.err = (uint32_t)id_check_head(pl, pbytes, &S.mode, &S.tbytes, S.bm, &S.hdr1);
        if (!S.err && (uint64_t)S.tbytes != toff[b + 1] - toff[b]) S.err = ID_E_SIZE;
    }
    __syncthreads();
    if (S.err) { if (t == 0) atomicMin(errw, ((unsigned long long)b << 8) | S.err); return; }
    const uint32_t T = S.tbytes;
    if (S.mode == 0) {
        uint32_t nl = 0;
        for (uint32_t j = t; j < T; j += IP_T) { const uint8_t v = pl[ID_HEAD0 + j]; nl += v == '\n'; tx[j] = v; }
        if (nl) atomicAdd(&S.newlines, nl);
        __syncthreads();
        if (t == 0 && (S.newlines != m || (T && pl[ID_HEAD0 + T - 1u] != '\n'))) atomicMin(errw, ((unsigned long long)b << 8) | ID_E_TEXT);
        return;
    }
    const uint32_t h = S.hdr1, rest = pbytes - h;
    // the smallest code of what is wrong, as id_block_decode answers
    uint32_t e = ID_E_NONE, stext = 0, len = 0;
    if (t < ID_ROWS) e = id_code(id_load_row(pl + ID_HEAD1, S.bm, t, S.fc));
    e = id_min(e, id_code(id_check_strand(pl, m, t, &stext, &len)));
    if (e != ID_E_NONE) atomicMin(&S.verr, e);
    atomicAdd(&S.tsum, (unsigned long long)stext);
    atomicAdd(&S.lsum, (unsigned long long)len);
    __syncthreads();
    if (t == 0) { if (S.tsum != T) S.verr = id_min(S.verr, ID_E_SIZE); if (S.lsum != rest) S.verr = id_min(S.verr, ID_E_LENGTHS); }
    __syncthreads();
    if (S.verr != ID_E_NONE) { if (t == 0) atomicMin(errw, ((unsigned long long)b << 8) | S.verr); return; }
    uint32_t total;                                                // (the sums have been checked: both scans stay below 2^32)
    const uint32_t at = block_excl_scan_u32<IP_T>(len, S.scan, &total);
    const uint32_t tat = block_excl_scan_u32<IP_T>(stext, S.scan, &total);
    e = id_code(id_strand_decode(pl + h + at, len, S.fc, tx + tat, stext, id_strand_lines(m, t)));
    if (e != ID_E_NONE) atomicMin(&S.verr, e);
    __syncthreads();
    if (t == 0 && S.verr != ID_E_NONE) atomicMin(errw, ((unsigned long long)b << 8) | S.verr);
}

static const char *id_error_text(uint32_t e)
{
    switch (e) {
    case ID_E_MODE: return "its mode is neither 0 nor 1";
    case ID_E_SIZE: return "its sizes do not fit its mode or do not sum to its text bytes";
    case ID_E_BITMAP: return "its bitmap names a row past the last";
    case ID_E_ROW: return "a present row of its table does not sum to 4096";
    case ID_E_LENGTHS: return "its strand lengths do not sum to the rest of its payload";
    case ID_E_SHORT: return "a strand with lines is shorter than 4 bytes or than its lines, or one without lines is not empty";
    case ID_E_TRUNC: return "a strand ends before its last event";
    case ID_E_CONTEXT: return "a symbol is coded in a row that is absent or in a slot that is empty";
    case ID_E_END: return "a strand does not end in the state and at the byte it must";
    case ID_E_PREV: return "a token matches or counts on from a token that the previous line does not have";
    case ID_E_VALUE: return "a number is above 999999999 or a difference is 0";
    case ID_E_TEXT: return "its lines do not fill its text bytes exactly";
    case ID_E_EMPTY: return "a literal holds no byte";
    }
    return "unknown error";
}

// ------------------------------------------------------------------------------------------------ packing: the blocks of n lines
// the blocks alone (no file header) of the n lines that start at d_text + t0 and end at d_text + t1, nls their line index (nls[-1] + 1 == t0) -> d_out[0 .. *n_out);
// d_out == nullptr: the size alone.  block0: the number of the first of them, for the message
static int harc_idpack_run(harc_amd_ctx *c, const char *d_text, const uint64_t *nls, uint64_t t0, uint64_t t1, uint64_t n, uint32_t RB, uint8_t *d_out, uint64_t out_capacity,
                           uint64_t *n_out, uint64_t block0, PackStats *st)
{
    const uint8_t *text = (const uint8_t *)d_text;
    const uint64_t nev = (t1 - t0) + 2ull * n;
    uint16_t *events = nullptr; uint8_t *slabs = nullptr, *heads = nullptr; uint64_t *sat = nullptr, *btext = nullptr;
    // (sat holds ID_STRANDS entries a block: that many fewer blocks a call.  err[0] is lowered by atomicMin: all ones says that no block is too long)
    return pack_run(c, "idpack", id_blocks(n, RB), 0x7FFFFFF0ull / ID_STRANDS, t1 - t0, d_out, out_capacity, n_out, st,
        [&](const PackBlocks &B) -> int {
            const size_t nb = B.nb;
            RC_TRY(dalloc(c, &events, (size_t)nev)); RC_TRY(dalloc(c, &slabs, (size_t)(2ull * nev + 32ull * ID_STRANDS * nb))); RC_TRY(dalloc(c, &heads, (size_t)IP_HDR * nb));
            RC_TRY(dalloc(c, &sat, (size_t)ID_STRANDS * nb)); RC_TRY(dalloc(c, &btext, nb));
            HIP_TRY(hipMemsetAsync(B.err, 0xFF, 4, c->stream));
            return HARC_AMD_OK;
        },
        [&](const PackBlocks &B) {
            hipLaunchKernelGGL(k_ip_encode, harc_fold256(B.nb), dim3(IP_T), 0, c->stream, text, nls, t0, n, RB, B.nb, events, slabs, heads, sat, btext, B.bsize, B.bmode, B.err);
        },
        [&](const unsigned int *err, PackStats *stats) {
            if (err[0] != 0xFFFFFFFFu) { harc_set_error("idpack: the text of block %llu is longer than %u bytes", (unsigned long long)(block0 + err[0] - 1), ID_MAX_BLOCK_TEXT); return HARC_AMD_EINVAL; }
            if (err[1]) { harc_set_error("idpack: %u strands did not fit their scratch", err[1]); return HARC_AMD_EINTERNAL; }
            if (stats) stats->mode[0] += err[2];
            return HARC_AMD_OK;
        },
        [&](const PackBlocks &B, uint8_t *out) {
            hipLaunchKernelGGL(k_ip_gather, harc_fold256(B.nb), dim3(IP_T), 0, c->stream, text, B.nb, (const uint8_t *)slabs, (const uint8_t *)heads, (const uint64_t *)sat,
                               (const uint64_t *)btext, (const uint32_t *)B.bsize, (const uint32_t *)B.bmode, (const uint64_t *)B.boff, out);
        });
}
// the line index of text_bytes > 0 bytes that end in a newline.  Pool memory: the caller brackets it
static int ip_index(harc_amd_ctx *c, const char *who, const char *d_text, uint64_t text_bytes, const uint64_t **nls, uint64_t *lines)
{
    char lastch = 0;
    HIP_TRY(hipMemcpyAsync(&lastch, d_text + text_bytes - 1, 1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (lastch != '\n') { harc_set_error("%s: the last line of the id text does not end in a newline", who); return HARC_AMD_EINVAL; }
    return build_line_index(c, d_text, text_bytes, nls, lines);
}
static uint32_t ip_rb(uint32_t lines_per_block) { return lines_per_block ? lines_per_block : ID_DEFAULT_RB; }

extern "C" uint64_t harc_amd_idpack_bound(uint64_t text_bytes, uint64_t n_lines, uint32_t lines_per_block) { return id_bound(text_bytes, n_lines, ip_rb(lines_per_block)); }

extern "C" int harc_amd_idpack_device(harc_amd_ctx *c, const char *d_text, uint64_t text_bytes, uint32_t lines_per_block, int32_t flags, uint8_t *d_out, uint64_t out_capacity,
                                      uint64_t *n_out)
{
    const uint32_t rb = ip_rb(lines_per_block);
    uint64_t n = 0;
    return pack_device("idpack", c, !text_bytes || d_text, (flags & HARC_AMD_IDPACK_NO_HEADER) ? 0 : ID_FILE_HEADER, d_out, out_capacity, n_out,
        [] { return HARC_AMD_OK; },                                // (every number of lines per block is a geometry)
        [&](uint8_t *o, uint64_t cap, uint64_t *nblk, PackStats *st) -> int {
            if (!text_bytes) return HARC_AMD_OK;
            PoolScope scope(c);                                    // the line index
            const uint64_t *nls = nullptr;
            RC_TRY(ip_index(c, "idpack_device", d_text, text_bytes, &nls, &n));
            return harc_idpack_run(c, d_text, nls, 0, text_bytes, n, rb, o, cap, nblk, 0, st);
        },
        [&](uint8_t *h) { id_file_header(h, rb, n, text_bytes); },
        [&](const PackStats &st, uint64_t bytes) {
            fprintf(stderr, "[idpack] device call: %llu bytes of text -> %llu bytes in %llu blocks (%llu stored), kernels %.3f ms (%.2f GB/s of text)\n", (unsigned long long)text_bytes,
                    (unsigned long long)bytes, (unsigned long long)st.blocks, (unsigned long long)st.mode[0], 1e3 * st.seconds, st.seconds > 0 ? 1e-9 * (double)st.text / st.seconds : 0.0);
        });
}

// ------------------------------------------------------------------------------------------------ unpacking
// the 32 bytes at h of a packed form of n_bytes bytes
static int ip_parse_header(const char *who, const uint8_t *h, uint64_t n_bytes, PackHeader *H)
{
    if (!id_magic_ok(h)) { harc_set_error("%s: no packed id file: its first 8 bytes are not the magic HARCI1", who); return HARC_AMD_EINVAL; }
    H->rb = qv_le32(h + 8); H->n = qv_le64(h + 16); H->text = qv_le64(h + 24);
    if (qv_le32(h + 12)) { harc_set_error("%s: bytes 12..15 of the header are not 0", who); return HARC_AMD_EINVAL; }
    if (H->n == 0) {
        if (H->rb || H->text || n_bytes != ID_FILE_HEADER) { harc_set_error("%s: the header announces no lines, but a block size, text or %llu bytes behind it", who, (unsigned long long)(n_bytes - ID_FILE_HEADER)); return HARC_AMD_EINVAL; }
        H->nb = 0;
        return HARC_AMD_OK;
    }
    if (H->rb < 1) { harc_set_error("%s: the header names 0 lines per block", who); return HARC_AMD_EINVAL; }
    H->nb = id_blocks(H->n, H->rb);
    if (H->nb > (n_bytes - ID_FILE_HEADER) / (4u + ID_HEAD0)) { harc_set_error("%s: the header announces %llu blocks, %llu bytes cannot hold them", who, (unsigned long long)H->nb, (unsigned long long)n_bytes); return HARC_AMD_EINVAL; }
    if (H->text < H->n || H->text > H->nb * (uint64_t)ID_MAX_BLOCK_TEXT) { harc_set_error("%s: the header announces %llu lines in %llu bytes of text", who, (unsigned long long)H->n, (unsigned long long)H->text); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}
// the prefix rule (the text bytes of a block stand behind its payload bytes)
struct IdRule {
    static __host__ __device__ int prefix(const PackHeader &, uint64_t, const uint8_t *q, uint64_t left, uint64_t text_left, uint64_t *pb, uint64_t *tb)
    {
        return id_prefix(q, left, text_left, pb, tb);
    }
};
static const PackFormat ID_FORMAT = {
    "id", "id", "HARC_AMD_IDPACK_PIECE", 8, ID_PREFIX, ip_parse_header, IdRule::prefix, pack_walk_device<IdRule>,
    [](harc_amd_ctx *c, const uint8_t *d_blocks, const uint64_t *d_off, const uint64_t *d_toff, uint32_t nb, uint64_t n, const PackHeader &H, char *d_text, unsigned long long *d_errw) {
        hipLaunchKernelGGL(k_ip_decode, harc_fold256(nb), dim3(IP_T), 0, c->stream, d_blocks, d_off, d_toff, nb, n, H.rb, (uint8_t *)d_text, d_errw);
    },
    id_error_text,
};

extern "C" int harc_amd_idunpack_device(harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, char *d_text, uint64_t out_capacity, uint64_t *n_out)
{
    return pack_unpack_device(ID_FORMAT, c, d_packed, n_bytes, d_text, out_capacity, n_out);
}

// ------------------------------------------------------------------------------------------------ the same in a row on the host: what the kernels are held to
extern "C" int harc_amd_idpack_host(const char *text, uint64_t text_bytes, uint32_t lines_per_block, int32_t flags, uint8_t *out, uint64_t cap, uint64_t *n_out)
{
    if ((text_bytes && !text) || !n_out) { harc_set_error("idpack_host: bad arguments"); return HARC_AMD_EINVAL; }
    if (text_bytes && text[text_bytes - 1] != '\n') { harc_set_error("idpack_host: the last line of the id text does not end in a newline"); return HARC_AMD_EINVAL; }
    const uint32_t rb = ip_rb(lines_per_block);
    const uint64_t head = (flags & HARC_AMD_IDPACK_NO_HEADER) ? 0 : ID_FILE_HEADER;
    std::vector<IdWork> W(1);
    std::vector<uint16_t> events; std::vector<uint8_t> slabs, blk;
    uint64_t at = head, n = 0, a = 0, block = 0;
    while (a < text_bytes) {
        uint64_t e = a; uint32_t m = 0;
        while (e < text_bytes && m < rb) { const char *q = (const char *)memchr(text + e, '\n', (size_t)(text_bytes - e)); e = (uint64_t)(q - text) + 1; m++; }
        if (e - a > ID_MAX_BLOCK_TEXT) { harc_set_error("idpack: the text of block %llu is longer than %u bytes", (unsigned long long)block, ID_MAX_BLOCK_TEXT); return HARC_AMD_EINVAL; }
        const uint32_t tb = (uint32_t)(e - a);
        events.resize((size_t)id_block_events(tb, m)); slabs.resize((size_t)id_block_slabs(tb, m)); blk.resize((size_t)4 + ID_HEAD0 + tb);
        const uint32_t sz = id_block_encode((const uint8_t *)text + a, tb, m, W[0], events.data(), slabs.data(), blk.data(), blk.size(), nullptr);
        if (!sz) { harc_set_error("idpack_host: a strand did not fit its scratch"); return HARC_AMD_EINTERNAL; }
        if (out && at + sz <= cap) memcpy(out + at, blk.data(), sz);
        at += sz; n += m; a = e; block++;
    }
    *n_out = at;
    if (!out) return HARC_AMD_OK;
    if (cap < at) { harc_set_error("idpack_host: the packed form takes %llu bytes, the buffer holds %llu", (unsigned long long)at, (unsigned long long)cap); return HARC_AMD_EINVAL; }
    if (head) id_file_header(out, rb, n, text_bytes);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idunpack_host(const uint8_t *packed, uint64_t n_bytes, char *text, uint64_t cap, uint64_t *n_out)
{
    std::vector<IdWork> W(1);
    return pack_unpack_host(ID_FORMAT, packed, n_bytes, (uint8_t *)text, cap, n_out,
                            [&](const PackHeader &, const uint8_t *pl, uint32_t pb, uint32_t m, uint8_t *tx) { return id_block_decode(pl, pb, m, W[0], tx); });
}

// ------------------------------------------------------------------------------------------------ the files
// The text goes through the ring in byte ranges of about `piece_blocks` blocks of ids of 80 bytes (4 KiB .. 256 MiB).  The line index of what has arrived says how
// many whole blocks it holds: they are packed, at most piece_blocks and at most IP_CALL_TEXT bytes of text a call (one block where a block alone is longer), and the
// rest is carried to the front of the next range (CarriedText of fileio.h, whose steps of a turn over whole lines this loop is made of).  The event scratch and the slabs are five bytes per byte of text: 1.25 GiB a
// call with ids of any length, and 5 GiB in the one case that cannot be cut, a single block of the 2^30 bytes a block may hold
extern "C" int harc_amd_idpack_files(const harc_amd_params *params, const char *id_path, const char *out_path)
{
    if (!params || !id_path || !out_path) { harc_set_error("idpack_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t isz = 0;
    if (!file_size(id_path, &isz)) { harc_set_error("cannot open %s", id_path); return HARC_AMD_EIO; }
    OutFileGuard outguard{ out_path };
    if (isz) {                                                    // before a device is touched
        bool closed = false;
        RC_TRY(last_byte_is_newline(id_path, &closed));
        if (!closed) { harc_set_error("idpack_files: the last line of %s does not end in a newline", id_path); return HARC_AMD_EINVAL; }
    }
    const uint32_t rb = (uint32_t)env_u64("HARC_AMD_IDPACK_BLOCK", ID_DEFAULT_RB);
    const uint64_t piece_blocks = env_u64(ID_FORMAT.piece_env, ID_FORMAT.piece_default), call_text = env_u64("HARC_AMD_IDPACK_CALL_TEXT", IP_CALL_TEXT);
    uint64_t piece = piece_blocks * rb * 80ull;
    if (piece < 4096) piece = 4096;
    if (piece > ((uint64_t)256 << 20)) piece = (uint64_t)256 << 20;
    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom g[2];                                                // the feeder's and the drain's
    RC_TRY(ring_split(c, 2, 8, ID_FORMAT.ring, g));
    CarriedText txt(c); DevBuf out{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0;
    PackStats st;
    uint64_t at = ID_FILE_HEADER, n = 0, nb = 0; int npieces = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)id_bound(isz, isz, rb), &g[1], true));      // (no more lines than bytes)
        const Pieces pieces = byte_pieces(0, isz, piece);
        FileFeeder feed(c, id_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, g[0]));
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t len = pieces[p].second - pieces[p].first, total = txt.carry + len; const bool lastp = p + 1 == pieces.size();
            RC_TRY(txt.take(feed, p, len, &t_read));                                         // the carried bytes sit at its front
            PoolScope piece_scope(c);
            LineTurn t;
            RC_TRY(txt.index(total, lastp, &t));
            const char *d_ids = t.text; const uint64_t *nls = t.nls;
            const uint64_t lines = lastp ? t.whole : t.whole / rb * rb;                      // whole lines, then whole blocks
            uint64_t cut = 0;
            for (uint64_t l0 = 0; l0 < lines;) {
                // at most piece_blocks blocks a call and, by the line index, no more than IP_CALL_TEXT bytes of text unless one block alone is longer
                uint64_t m = lines - l0 < piece_blocks * rb ? lines - l0 : piece_blocks * rb, end = 0;
                for (;;) {
                    RC_TRY(txt.line_end(nls, l0 + m, &end));
                    if (end - cut <= call_text || m <= rb) break;
                    const uint64_t half = (id_blocks(m, rb) / 2) * rb;
                    m = half < rb ? rb : half;
                }
                RC_TRY(dev_reserve(&out, (size_t)(id_bound(end - cut, m, rb) - ID_FILE_HEADER)));
                uint64_t nblk = 0;
                RC_TRY(harc_idpack_run(c, d_ids, nls + l0, cut, end, m, rb, (uint8_t *)out.p, out.cap, &nblk, nb, &st));
                { const double t0 = mono_now(); RC_TRY(drain.put(out.p, (size_t)nblk, at)); t_write += mono_now() - t0; }
                at += nblk; n += m; nb += id_blocks(m, rb); npieces++;
                l0 += m; cut = end;
            }
            RC_TRY(txt.carry_behind(cut, total));                                            // (nothing, or not one whole block yet: the piece grows by the next one)
        }
        uint8_t h[ID_FILE_HEADER];
        id_file_header(h, rb, n, isz);
        RC_TRY(drain.put_host(h, ID_FILE_HEADER, 0));
        drain.set_final_size(at);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    if (tlog) fprintf(stderr, "[idpack] %llu bytes of text -> %llu bytes in %llu blocks (%llu stored), %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers\n",
                      (unsigned long long)isz, (unsigned long long)at, (unsigned long long)nb, (unsigned long long)st.mode[0], npieces, st.seconds, t_read, t_write);
    outguard.ok = true;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path)
{
    return pack_unpack_files(ID_FORMAT, params, packed_path, out_path);
}

extern "C" int harc_amd_idunpack_range_files(const harc_amd_params *params, const char *packed_path, const char *out_path, uint64_t first_line, uint64_t n_lines)
{
    const uint64_t range[2] = { first_line, n_lines };
    return pack_unpack_files(ID_FORMAT, params, packed_path, out_path, nullptr, 0, range);
}
